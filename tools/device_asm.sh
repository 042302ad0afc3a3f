#!/usr/bin/env bash
# Dump the normalised gfx950 device assembly of every csrc/*.hip of a source tree, for comparing two trees:
#
#     tools/device_asm.sh <tree> <outdir>      # <tree> is a checkout of this repository
#     diff -r <outdir-of-parent> <outdir-of-this-tree>
#
# Each file is compiled with the flags its object gets from csrc/Makefile (asked of `make -n`, so per-file additions such
# as -ffp-contract=off follow), with `-c -o x.o` replaced by `--cuda-device-only -S -o <outdir>/x.s`.  The one thing a
# host-only edit changes in that output is the compilation-unit hash `__hip_cuid_<hex>`; it is masked.  A refactor that
# leaves device code alone therefore gives identical directories; after a kernel is re-parameterised, only the lines
# that carry its (mangled) name differ.  Needs hipcc, no GPU.
set -euo pipefail
tree=$(cd "${1:?usage: device_asm.sh <tree> <outdir>}" && pwd)
mkdir -p "${2:?usage: device_asm.sh <tree> <outdir>}"
out=$(cd "$2" && pwd)
cd "$tree/flair_amd/csrc"
jobs=${JOBS:-8}
for src in *.hip; do
    obj=${src%.hip}.o
    cmd=$(make -n -B "$obj" | grep -- " -c $src ")
    cmd=${cmd/ -c $src -o $obj/ --cuda-device-only -S $src -o $out/${src%.hip}.s}
    while [ "$(jobs -rp | wc -l)" -ge "$jobs" ]; do wait -n; done
    ( $cmd && sed -E -i 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out/${src%.hip}.s" ) &
done
while [ "$(jobs -rp | wc -l)" -gt 0 ]; do wait -n; done      # wait -n: a failed compile ends the script (set -e)
echo "device assembly of $(ls "$out"/*.s | wc -l) files in $out"
