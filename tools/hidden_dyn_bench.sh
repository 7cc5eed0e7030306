#!/bin/bash
# hidden_dyn_bench.sh <parent libd2d_hip.so> <parent chainprof.so> [out dir] -- runs on the GPU box: the persistent closed loop whose hidden
# steps skip the dynamic-grid stage (dyn_skip in csrc/d2d_hip.hip) against the parent commit's library, the two alternating
# (D2D_LIB).  The lines, the rounds and the limits are those of tools/hidden_obs_bench.sh, which this script runs into its own
# directory (PARTS=main / PARTS=other may run as calls of their own); tools/hidden_dyn_collect.py condenses it into
# profiles/hidden_dyn.json.
#   PARTS=forms ALT_LIB=<libd2d_hip.so of the other form>: the 600 / 300 line alone, parent, this tree and ALT_LIB alternating -- how
#   the form of the change was chosen (one instantiation with wave-uniform branches against a second instantiation of run_env).
# Every step runs under its own time limit and the script ends at the first step that fails.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${3:-$ROOT/bench_outputs/hidden_dyn}
PARTS=${PARTS:-main other}
if [[ " $PARTS " == *" main "* || " $PARTS " == *" other "* ]]; then
  PARTS=$(echo " $PARTS " | sed 's/ forms / /') bash "$ROOT/tools/hidden_obs_bench.sh" "$1" "$2" "$OUT"
fi
if [[ " $PARTS " == *" forms "* ]]; then
  PARENT=$(readlink -f "$1")
  ALT=$(readlink -f "$ALT_LIB")
  THIS=$ROOT/gym-drone2d-activeperception_amd/csrc/libd2d_hip.so
  for f in "$PARENT" "$ALT" "$THIS"; do [ -f "$f" ] || { echo "missing $f"; exit 2; }; done
  mkdir -p "$OUT"
  cd "$ROOT"
  for r in $(seq "${ROUNDS:-6}"); do
    for which in parent this alt; do
      case $which in parent) lib=$PARENT ;; this) lib=$THIS ;; alt) lib=$ALT ;; esac
      name=forms_600_300_${which}_$r
      echo "== $name"
      D2D_LIB=$lib timeout -k 10 240 python3 bench.py --gpus 1 --steps 600 --warmup 300 --no-cpu-baseline --large 0 \
        > "$OUT/$name.out" 2> "$OUT/$name.err" || { echo "FAILED $name (exit $?)"; tail -5 "$OUT/$name.err"; exit 1; }
    done
  done
fi
echo "hidden_dyn_bench: done, $OUT"
