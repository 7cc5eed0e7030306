#!/usr/bin/env python3
"""What obs['scan'] (VecDrone2DEnv(..., scan_obs=True), include/d2d_scan.h) costs a learner on an action
stream.  For each planner cell two streams live in one process and take turns, run for run, so that both see the same clocks and the
same neighbours:

  off    scan_obs=False: the stream of before
  on     scan_obs=True: the same step, a copy of the pose in front of it and d2d_scan_update behind it

Shape: --slots 4096, 10 agents (BASELINE config 2's parameters), Primitive / CVM and Jerk_Primitive / CVM, gaze='external', the
constant action 0, --warmup steps each, then --reps times (off, on) runs of --steps steps each between HIP events and on the wall
clock, the order rotating from repetition to repetition; a turn every 4 steps, as the stream's default has it.  Episodes end and
slots refill inside the runs, as they do for a learner.  Two launches are timed alone on the `on` env of each cell, --launches calls
each between HIP events: d2d_scan_update with the step counters moved on by hand between calls, so that every env is due every
time (the bump is timed separately and subtracted), and d2d_run_stages(AGENTS | RAYCAST), the raycast stage of bench.py.

python tools/scan_obs_bench.py --out profiles/scan_obs.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)
CELLS = {'Primitive-CVM': 'Primitive', 'Jerk-CVM': 'Jerk_Primitive'}


def timed(torch, hip, n, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    hip.sync()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out')
    args = ap.parse_args()
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A, _lib, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    cells = {}
    for cell, planner in CELLS.items():
        streams = {}
        for variant in ('off', 'on'):
            env = vec_env.VecDrone2DEnv(pkg.Params(planner=planner, **WORLD), args.slots, backend=hip, planner=planner, device_plugins=True,
                                        gaze='external', worlds='device', scan_obs=variant == 'on')
            streams[variant] = env.action_stream(refill_every=4)
        act = torch.zeros(args.slots, dtype=torch.float64, device=hip.device)
        for stream in streams.values():
            for _ in range(args.warmup):
                stream.step(act)
        hip.sync()
        runs = []
        for rep in range(args.reps):
            order = list(streams) if rep % 2 == 0 else list(streams)[::-1]
            for variant in order:
                stream = streams[variant]
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
                                 wall_steps_a_second=args.steps / wall, microseconds_a_step=sec / args.steps * 1e6,
                                 finished=stream.finished_now(), channels=sorted(obs)))
        median, spread = {}, {}
        for variant in streams:
            rates = sorted(r['steps_a_second'] for r in runs if r['variant'] == variant)
            median[variant] = rates[len(rates) // 2]
            spread[variant] = (rates[-1] - rates[0]) / median[variant]
        # the two launches alone, on the `on` stream's env as the runs left it
        env = streams['on'].env
        counters = env.state.counters[:, A.C_STEPS]
        bump = torch.ones_like(counters)
        kinds = torch.bincount(env.ray_kind.reshape(-1).long(), minlength=4).tolist()

        def scan_launch():
            counters.add_(bump)
            env._scan_update()
        timed(torch, hip, 10, scan_launch)
        scan_us = timed(torch, hip, args.launches, scan_launch)
        bump_us = timed(torch, hip, args.launches, lambda: counters.add_(bump))
        due = int((env.scan['last_step'] == counters - args.launches).sum())
        stage = lambda: hip.run_stages(env.cfg, env._st, A.ST_AGENTS | A.ST_RAYCAST)      # noqa: E731
        timed(torch, hip, 10, stage)
        stage_us = timed(torch, hip, args.launches, stage)
        cells[cell] = dict(runs=runs, median_steps_a_second=median, spread_over_median=spread, on_over_off=median['on'] / median['off'],
                           rays_by_kind_at_the_end_of_the_runs=kinds,
                           launches_alone=dict(launches=args.launches, scan_microseconds_with_the_counter_bump=scan_us,
                                               microseconds_of_the_bump=bump_us, scan_microseconds=scan_us - bump_us,
                                               envs_updated_by_the_last_timed_scan_launch=due,
                                               raycast_stage_microseconds=stage_us))
        for stream in streams.values():
            stream.close()
        del streams, env
    out = dict(tool='tools/scan_obs_bench.py', device=torch.cuda.get_device_name(0), slots=args.slots, steps=args.steps, warmup=args.warmup,
               reps=args.reps, world=WORLD, cells=cells)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
