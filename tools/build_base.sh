#!/usr/bin/env bash
# tools/build_base.sh [rev] -- build libdsm.so of git revision `rev` (default HEAD) into
# ab/libdsm_${NAME:-base}.so, for an A/B against the working tree with tools/ab_lib.sh.
# The revision is built by its own Makefile, so its own list of units: a revision from before
# the engine was split into units builds as it did then.
set -e
REV=${1:-HEAD}
T=$(mktemp -d)
git archive "$REV" hp-assignment-2_amd include | tar -x -C "$T"
make -s -C "$T/hp-assignment-2_amd" -j8 libdsm.so 2>"$T/warn.txt" || { cat "$T/warn.txt"; exit 1; }
mkdir -p ab
cp "$T/hp-assignment-2_amd/libdsm.so" "ab/libdsm_${NAME:-base}.so"
rm -rf "$T"
echo "ab/libdsm_${NAME:-base}.so <- $REV"
