#!/usr/bin/env python3
"""What obs['swep_map'] as a channel of its own (VecDrone2DEnv(..., swept_obs=True), include/d2d_swept.h) costs a
learner on an action stream.  One variant per process (--variant), every run kept:

  off    swept_obs=False: the stream of before, whose steps are the persistent kernel (closed_loop(1, freeze_done=True))
  on     swept_obs=True: one launch per stage -- perceive, d2d_swept_mark, plan, act, d2d_swept_crop

Run from a tree of the parent commit, `off` is the parent's own figure (the keyword does not exist there: --variant parent builds the
env without it).  Shape: --slots 4096, 10 agents (BASELINE config 2's parameters), Primitive / CVM, gaze='external', the constant action
0, --warmup steps, then --reps runs of --steps steps each between HIP events and on the wall clock; a turn every 4 steps, as the
stream's default has it.  Episodes end and slots refill inside the runs, as they do for a learner.

python tools/swept_obs_bench.py --variant on --out swept_on.json"""
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
    ap.add_argument('--variant', choices=('parent', 'off', 'on'), required=True)
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _lib, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    kw = {} if args.variant == 'parent' else dict(swept_obs=args.variant == 'on')
    env = vec_env.VecDrone2DEnv(pkg.Params(**WORLD), args.slots, backend=hip, planner='Primitive', device_plugins=True, gaze='external',
                                worlds='device', **kw)
    stream = env.action_stream(refill_every=4)
    act = torch.zeros(args.slots, dtype=torch.float64, device=hip.device)
    for _ in range(args.warmup):
        stream.step(act)
    hip.sync()
    runs = []
    for rep in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.steps):
            obs = stream.step(act)[0]
        b.record()
        hip.sync()
        wall = time.perf_counter() - t0
        sec = a.elapsed_time(b) * 1e-3
        runs.append(dict(rep=rep, seconds=sec, wall_seconds=wall, steps_a_second=args.steps / sec, wall_steps_a_second=args.steps / wall,
                         env_steps_a_second=args.steps * args.slots / sec, microseconds_a_step=sec / args.steps * 1e6,
                         finished=stream.finished_now()))
    rates = [r['steps_a_second'] for r in runs]
    out = dict(tool='tools/swept_obs_bench.py', variant=args.variant, device=torch.cuda.get_device_name(0), slots=args.slots, steps=args.steps,
               warmup=args.warmup, world=WORLD, swep_map_is_local_map=obs['swep_map'].data_ptr() == obs['local_map'].data_ptr(), runs=runs,
               median_steps_a_second=sorted(rates)[len(rates) // 2], span_steps_a_second=max(rates) - min(rates))
    stream.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
