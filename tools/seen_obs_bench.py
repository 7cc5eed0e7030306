#!/usr/bin/env python3
"""What obs['age_map'] (VecDrone2DEnv(..., seen_obs=True), include/d2d_seen.h) costs a learner on an action
stream.  Two streams live in one process and take turns, run for run, so that both see the same clocks and the same neighbours:

  off    seen_obs=False: the stream of before, whose steps are the persistent kernel (closed_loop(1, freeze_done=True))
  on     seen_obs=True: the same step, and d2d_seen_update behind it

Shape: --slots 4096, 10 agents (BASELINE config 2's parameters), Primitive / CVM, gaze='external', the constant action 0, --warmup steps
each, then --reps times (off, on) runs of --steps steps each between HIP events and on the wall clock; a turn every 4 steps, as the
stream's default has it.  Episodes end and slots refill inside the runs, as they do for a learner.  The launch alone is timed too:
--launches calls of d2d_seen_update on the `on` stream's env with its step counters moved on by hand between calls, so that every
env is due every time.

python tools/seen_obs_bench.py --out profiles/seen_obs.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(planner='Primitive', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=100)     # (the table ends at call 408: 100 + 2 x 100 stays below)
    ap.add_argument('--out')
    args = ap.parse_args()
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A, _lib, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    streams = {}
    for variant in ('off', 'on'):
        env = vec_env.VecDrone2DEnv(pkg.Params(**WORLD), args.slots, backend=hip, planner='Primitive', device_plugins=True, gaze='external',
                                    worlds='device', seen_obs=variant == 'on')
        streams[variant] = env.action_stream(refill_every=4)
    act = torch.zeros(args.slots, dtype=torch.float64, device=hip.device)
    for stream in streams.values():
        for _ in range(args.warmup):
            stream.step(act)
    hip.sync()
    runs = []
    for rep in range(args.reps):
        for variant, stream in streams.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.steps):
                obs = stream.step(act)[0]
            b.record()
            hip.sync()
            wall = time.perf_counter() - t0
            sec = a.elapsed_time(b) * 1e-3
            runs.append(dict(variant=variant, rep=rep, seconds=sec, wall_seconds=wall, steps_a_second=args.steps / sec,
                             wall_steps_a_second=args.steps / wall, microseconds_a_step=sec / args.steps * 1e6, finished=stream.finished_now(),
                             channels=sorted(obs)))
    median = {}
    for variant in streams:
        rates = sorted(r['steps_a_second'] for r in runs if r['variant'] == variant)
        median[variant] = rates[len(rates) // 2]
    # the launch alone: every env is made due before every call
    env = streams['on'].env
    steps0 = env.state.counters[:, A.C_STEPS].clone()
    env.seen['last_call'].zero_()
    for k in range(10):
        env.state.counters[:, A.C_STEPS] = steps0 % 100 + k
        env._seen_update()
    hip.sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    env.seen['last_call'].zero_()
    bump = torch.ones_like(steps0)
    env.state.counters[:, A.C_STEPS] = steps0 % 100
    a.record()
    for k in range(args.launches):
        env.state.counters[:, A.C_STEPS].add_(bump)
        env._seen_update()
    b.record()
    hip.sync()
    launch_us = a.elapsed_time(b) * 1e3 / args.launches
    a.record()
    for k in range(args.launches):
        env.state.counters[:, A.C_STEPS].add_(bump)
    b.record()
    hip.sync()
    bump_us = a.elapsed_time(b) * 1e3 / args.launches
    due = int((env.seen['last_call'] == env.state.counters[:, A.C_STEPS] - args.launches + 1).sum())
    out = dict(tool='tools/seen_obs_bench.py', device=torch.cuda.get_device_name(0), slots=args.slots, steps=args.steps, warmup=args.warmup,
               world=WORLD, runs=runs, median_steps_a_second=median, on_over_off=median['on'] / median['off'],
               launch_alone=dict(launches=args.launches, microseconds_with_the_counter_bump=launch_us, microseconds_of_the_bump=bump_us,
                                 microseconds=launch_us - bump_us, envs_updated_by_the_last_timed_launch=due))
    for stream in streams.values():
        stream.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
