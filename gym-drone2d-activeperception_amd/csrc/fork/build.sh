#!/bin/bash
# Builds libd2d_fork.so (the slot fork: kernel + C ABI of include/d2d_fork.h) for gfx950, in-tree next to its sources.  The flags of
# csrc/tracks/build.sh (a pure copy has no arithmetic for -ffp-contract=off to matter to; the libraries are built alike).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -shared \
  -Wall -Wno-unused-function ${D2D_EXTRA_FLAGS:-} \
  -o ${D2D_OUT:-libd2d_fork.so} d2d_fork.hip
echo "built $(pwd)/${D2D_OUT:-libd2d_fork.so}"
