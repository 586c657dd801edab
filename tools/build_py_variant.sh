#!/usr/bin/env bash
# tools/build_py_variant.sh <name> <python-file> -- libdsm.so from the working tree with the
# python script applied to a scratch copy of csrc/ (it gets the copy's csrc path as argv[1])
# into ab/libdsm_<name>.so, EXTRA's hipcc flags on every unit (kernel-variant A/B; the edits
# never touch the tree).  The units, flags and link line are the Makefile's.
set -e
NAME=$1; PY=$2
T=$(mktemp -d)
cp -r hp-assignment-2_amd/csrc include "$T/"
python3 "$PY" "$T/csrc"
mkdir -p ab
make -s -C hp-assignment-2_amd -j8 SRC="$T/csrc" INC="$T/include" BUILD="$T/build" EXTRA="${EXTRA:-}" \
    LIB="$PWD/ab/libdsm_$NAME.so" "$PWD/ab/libdsm_$NAME.so" 2>"$T/warn.txt" || { cat "$T/warn.txt"; exit 1; }
rm -rf "$T"
echo "ab/libdsm_$NAME.so"
