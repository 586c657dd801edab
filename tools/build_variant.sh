#!/usr/bin/env bash
# tools/build_variant.sh <name> <sed-expr> [<sed-expr> ...] -- build libdsm.so from the
# working tree with sed edits applied to csrc/$FILE (default dsm_sim.hip, the transition kernel;
# tools/README.md says which unit holds what) into ab/libdsm_<name>.so, EXTRA's hipcc flags on
# every unit (kernel-variant A/B with tools/ab_lib.sh; the edits never touch the tree).
# The units, flags and link line are the Makefile's.
set -e
NAME=$1; shift
T=$(mktemp -d)
cp -r hp-assignment-2_amd/csrc include "$T/"
for e in "$@"; do sed -i "$e" "$T/csrc/${FILE:-dsm_sim.hip}"; done
mkdir -p ab
make -s -C hp-assignment-2_amd -j8 SRC="$T/csrc" INC="$T/include" BUILD="$T/build" EXTRA="${EXTRA:-}" \
    LIB="$PWD/ab/libdsm_$NAME.so" "$PWD/ab/libdsm_$NAME.so" 2>"$T/warn.txt" || { cat "$T/warn.txt"; exit 1; }
grep -i "spill\|occupancy" "$T/warn.txt" | head -5 || true
rm -rf "$T"
echo "ab/libdsm_$NAME.so"
