#!/bin/bash
# hidden_obs_bench.sh <parent libd2d_hip.so> <parent chainprof.so> [out dir] -- runs on the GPU box, ONE call: the persistent closed loop
# whose hidden steps skip the observation stage (hidden_stages in csrc/d2d_hip.hip) against the parent commit's library,
# the two alternating (D2D_LIB) as in tools/plan_fold_bench.sh:
#   bench.py --gpus 1 --steps 600 --warmup 300 --no-cpu-baseline --large 0     six runs per library
#   bench.py --steps 20 --warmup 5 --no-cpu-baseline --large 0                 six runs per library
#   bench.py --workload config3 / config4 / config5 --no-cpu-baseline --large 0    three runs each per library
#   tools/closed_loop_bench.py --envs 65536 --streams 1                        three runs per library
#   rocprofv3 --kernel-trace --stats of the 600 / 300 command                  once per library, a pass of its own (no counters)
#   tools/chain_prof.py                                                        once per library (the -DD2D_CHAIN_PROF builds)
# Every step runs under its own time limit and the script ends at the first step that fails: nothing is started on a GPU that a step
# before has faulted or hung.  tools/hidden_obs_collect.py condenses the output directory into profiles/hidden_obs.json.
# The parent's libraries: `git worktree add <dir> HEAD~1`, then csrc/build.sh there (and once more with D2D_OUT=chainprof.so
# D2D_EXTRA_FLAGS=-DD2D_CHAIN_PROF); this tree's chainprof.so is built the same way next to libd2d_hip.so.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$(readlink -f "$1")
PARENT_CP=$(readlink -f "$2")
OUT=${3:-$ROOT/bench_outputs/hidden_obs}
THIS=$ROOT/gym-drone2d-activeperception_amd/csrc/libd2d_hip.so
THIS_CP=$ROOT/gym-drone2d-activeperception_amd/csrc/chainprof.so
for f in "$PARENT" "$PARENT_CP" "$THIS" "$THIS_CP"; do [ -f "$f" ] || { echo "missing $f"; exit 2; }; done
ROUNDS=${ROUNDS:-6}
ROUNDS_OTHER=${ROUNDS_OTHER:-3}
PARTS=${PARTS:-main other}   # the two halves may run as calls of their own (PARTS=main, PARTS=other) into the same directory
mkdir -p "$OUT"
cd "$ROOT"
export TMPDIR=${TMPDIR:-/tmp}

lib_of() { [ "$1" = parent ] && echo "$PARENT" || echo "$THIS"; }
cp_of() { [ "$1" = parent ] && echo "$PARENT_CP" || echo "$THIS_CP"; }
# step <name> <seconds> <library> <command ...>: stdout to <name>.out, stderr to <name>.err; a failure ends the script
step() {
  local name=$1 limit=$2 lib=$3
  shift 3
  echo "== $name"
  D2D_LIB=$lib timeout -k 10 "$limit" "$@" > "$OUT/$name.out" 2> "$OUT/$name.err" || { echo "FAILED $name (exit $?)"; tail -5 "$OUT/$name.err"; exit 1; }
}

if [[ " $PARTS " == *" main "* ]]; then
for r in $(seq "$ROUNDS"); do
  for which in parent this; do
    step "bench_600_300_${which}_$r" 240 "$(lib_of $which)" python3 bench.py --gpus 1 --steps 600 --warmup 300 --no-cpu-baseline --large 0 &&
    step "bench_20_5_${which}_$r" 240 "$(lib_of $which)" python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --large 0
  done
done
for which in parent this; do
  step "chain_prof_$which" 300 "$(cp_of $which)" python3 tools/chain_prof.py
done
# the kernel trace: which instantiation the timed launches are, and their durations under the profiler
for which in parent this; do
  rm -rf "$OUT/ktrace_$which"
  step "ktrace_$which" 300 "$(lib_of $which)" rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ktrace_$which" -- \
    python3 bench.py --gpus 1 --steps 600 --warmup 300 --no-cpu-baseline --large 0 &&
  find "$OUT/ktrace_$which" -name '*kernel_stats.csv' -exec cp {} "$OUT/kernel_stats_$which.csv" \; &&
  find "$OUT/ktrace_$which" -name '*kernel_trace.csv' -exec sh -c 'grep -E "Kernel_Name|k_closed" "$1" > "$2"' _ {} "$OUT/kernel_trace_closed_$which.csv" \; &&
  rm -rf "$OUT/ktrace_$which"
done
fi
if [[ " $PARTS " == *" other "* ]]; then
for r in $(seq "$ROUNDS_OTHER"); do
  for which in parent this; do
    step "bench_config3_${which}_$r" 300 "$(lib_of $which)" python3 bench.py --workload config3 --no-cpu-baseline --large 0 &&
    step "bench_config4_${which}_$r" 300 "$(lib_of $which)" python3 bench.py --workload config4 --no-cpu-baseline --large 0 &&
    step "bench_config5_${which}_$r" 300 "$(lib_of $which)" python3 bench.py --workload config5 --no-cpu-baseline --large 0 &&
    step "closed_65536_${which}_$r" 300 "$(lib_of $which)" python3 tools/closed_loop_bench.py --envs 65536 --streams 1
  done
done
fi
echo "hidden_obs_bench: done, $OUT"
