#!/usr/bin/env bash
# tools/build_text_variant.sh <name> <hipcc flags...> -- libdsm.so with dsm_text.hip rebuilt
# with extra flags (e.g. -DPARSE_OCC=6) into ab/libdsm_<name>.so; the other objects are the
# tree's (hp-assignment-2_amd/build, built first where missing), linked by the Makefile's rule
set -e
NAME=$1; shift
T=$(mktemp -d)
make -s -C hp-assignment-2_amd -j8 libdsm.so 2>/dev/null
cp -rp hp-assignment-2_amd/build "$T/build"
rm -f "$T/build/dsm_text.o"
mkdir -p ab
make -s -C hp-assignment-2_amd BUILD="$T/build" EXTRA="$* -Rpass-analysis=kernel-resource-usage" \
    LIB="$PWD/ab/libdsm_$NAME.so" "$PWD/ab/libdsm_$NAME.so" 2>"$T/w.txt" || { cat "$T/w.txt"; exit 1; }
grep -A10 "parse_kernelILj32E" "$T/w.txt" | grep -E "VGPRs|Occupancy|Spill" | head -4
rm -rf "$T"
echo "ab/libdsm_$NAME.so"
