#!/bin/bash
# Builds libd2d_render.so (the renderer: kernels + C ABI of include/d2d_render.h and include/d2d_render_hooks.h) for gfx950, in-tree
# next to its sources.  The flags of csrc/tracks/build.sh:
#   -ffp-contract=off : no fused multiply-adds the rules do not spell out (the frame equals the host build and the numpy model bit for bit)
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -shared \
  -Wall -Wno-unused-function ${D2D_EXTRA_FLAGS:-} \
  -o ${D2D_OUT:-libd2d_render.so} d2d_render.hip
echo "built $(pwd)/${D2D_OUT:-libd2d_render.so}"
