#!/bin/bash
# sha256 of the device code object (gfx950 ELF, no host code) that a library's build.sh makes of a tree's .hip source.  Two trees
# whose kernels are the same print the same value: the check for a change that is meant to touch host code or dead code only.
#   tools/device_code_sha.sh [TREE [hip|worlds|metrics|rvo|jerk|gaze|seen|scan|tracks]] (default: this tree, e.g. a `git worktree` of the parent commit;
#                                                                      hip = csrc/build.sh, the others csrc/<name>/build.sh)
#   D2D_EXTRA_FLAGS=-DD2D_GAZE_EXACT_ONLY tools/device_code_sha.sh    (the libd2d_hip_exact.so build)
# -cuid pins the one symbol (__hip_cuid_<hash>) that otherwise differs from build to build.
set -euo pipefail
TREE=$(cd "${1:-$(dirname "$0")/..}" && pwd)
case "${2:-hip}" in
  hip) BUILD=build.sh ;;
  worlds | metrics | rvo | jerk | gaze | seen | scan | tracks) BUILD=$2/build.sh ;;
  *) echo "$0: library '$2': hip, worlds, metrics, rvo, jerk, gaze, seen, scan or tracks" >&2; exit 2 ;;
esac
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
D2D_OUT="$TMP/d2d_device.co" D2D_EXTRA_FLAGS="${D2D_EXTRA_FLAGS:-} --cuda-device-only --no-gpu-bundle-output -cuid=d2d -c" \
  bash "$TREE/gym-drone2d-activeperception_amd/csrc/$BUILD" > "$TMP/log" 2>&1 || { cat "$TMP/log" >&2; exit 1; }
sha256sum < "$TMP/d2d_device.co" | cut -d' ' -f1
