#!/bin/bash
# A/B(/C) builds of the headline kernel: $1 = source of variant A (default:
# HEAD's embed_fm.hip), the working tree's embed_fm.hip as B (extra hipcc
# flags for B in $BFLAGS, for A in $AFLAGS) and, when $CFLAGS is set, the
# working tree again with those flags as C (and with $DFLAGS as D).  Output:
# scripts/ab/librs_ab_{A,B,C,D}.so
# (diagnostics only; never loaded by the product).
# The working tree's embed_fm.hip gets the product's per-source flags
# (recommender_system_amd/_build.py SOURCE_FLAGS: the kernarg preload); A, an
# older source, gets only what $AFLAGS gives it.
# embed_fm.hip holds the FM kernel family alone (embed_fm_body.hpp: the body,
# from the working tree for every variant unless $1 lies in a directory that
# holds its own copy — a quoted include looks beside the including file
# first, so an A in an export of the parent's whole csrc is the parent's
# kernel, body included); beside it the libraries link what
# its entry points call: embed_fm_tiles.hip and capi.cpp.  (An A from before
# the kernel families were split out of embed_fm.hip does not compile against
# these headers: check out that commit and build its own A/B there.)
set -e
cd "$(dirname "$0")/.."
mkdir -p scripts/ab
rm -f scripts/ab/librs_ab_*.so
A=${1:-}
if [ -z "$A" ]; then A=$(mktemp -d)/embed_fm.hip; git show HEAD:recommender_system_amd/csrc/embed_fm.hip > "$A"; fi
C=recommender_system_amd/csrc
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include -I $C"
PRELOAD="-mllvm -amdgpu-kernarg-preload-count=14"
T=$(mktemp -d)
variant() {  # name, embed_fm source, flags
  hipcc $F $3 -x hip -c "$2" -o $T/embed_fm_$1.o &&
    hipcc $F ${3//$PRELOAD/} -shared $T/embed_fm_$1.o $C/embed_fm_tiles.hip $C/capi.cpp -o scripts/ab/librs_ab_$1.so
}
variant A "$A" "${AFLAGS:-}" &
variant B $C/embed_fm.hip "$PRELOAD ${BFLAGS:-}" &
if [ -n "${CFLAGS:-}" ]; then
  variant C $C/embed_fm.hip "$PRELOAD $CFLAGS" &
fi
if [ -n "${DFLAGS:-}" ]; then
  variant D $C/embed_fm.hip "$PRELOAD $DFLAGS" &
fi
wait
ls scripts/ab/librs_ab_A.so scripts/ab/librs_ab_B.so > /dev/null
