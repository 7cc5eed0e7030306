#!/bin/bash
# Builds libd2d_tracks.so (the tracker-forecast map as an observation channel: kernel + C ABI of include/d2d_tracks.h) for gfx950,
# in-tree next to its sources.  The flags of csrc/seen/build.sh:
#   -ffp-contract=off : no fused multiply-adds the reference does not perform (bit-exact parity)
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -shared \
  -Wall -Wno-unused-function ${D2D_EXTRA_FLAGS:-} \
  -o ${D2D_OUT:-libd2d_tracks.so} d2d_tracks.hip
echo "built $(pwd)/${D2D_OUT:-libd2d_tracks.so}"
