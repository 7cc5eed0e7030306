#!/usr/bin/env python3
"""Wall-clock cost of the Owl gaze policy (yaw_planner.py:151-222) as a device gaze stage.

  closed loop      env-steps/s of VecDrone2DEnv(..., gaze='Owl').closed_loop(--steps, auto_reset=True): the README configuration
                   (--envs x 10 agents), --reps repetitions on one batch after --warmup untimed steps
  ExperimentBatch  the host_gaze_rows r3 cfg (Owl + Primitive, tests/golden) over --envs map ids, one frozen episode each, one
                   closed_loop call per chunk
  episodes         --episodes stand-alone Experiment runs of the same cfg with the host policy gaze.Owl (per decision one
                   device-to-host mirror copy and the policy in Python): the only way to sweep Owl without the device stage

Times are wall clock around the call with a device synchronise before and after; worlds are built before the clock starts.
python tools/owl_gaze_bench.py --envs 4096 --steps 600 --warmup 300 --reps 3 --episodes 16"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README_CFG = dict(gaze_method='Owl', planner='Primitive', agent_number=10, agent_max_speed=20, agent_radius=15,
                  drone_max_speed=40, map_id=1)   # the README configuration = tests/golden/host_gaze_rows.npz r3_cfg


def closed_loop(envs, steps, warmup, reps, workers):
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import vec_env
    p = pkg.Params(**README_CFG)
    worlds = vec_env.build_worlds(p, envs, workers=workers)
    env = vec_env.VecDrone2DEnv(p, envs, planner='Primitive', device_plugins=True, gaze='Owl', worlds=worlds)
    env.closed_loop(warmup, auto_reset=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.closed_loop(steps, auto_reset=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out.append(dict(leg='closed_loop', gaze='Owl', envs=envs, steps=steps, warmup=warmup, wall_s=dt,
                        env_steps_per_s=envs * steps / dt))
    return out


def batch(envs, workers):
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import runner
    p = pkg.Params(debug=True, **README_CFG)
    p.render = False
    eb = runner.ExperimentBatch(p, envs, workers=workers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = eb.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = int(eb.env.state.counters[:, pkg._abi.C_STEPS].sum())
    return dict(leg='experiment_batch', gaze='Owl', envs=envs, wall_s=dt, env_steps=steps, env_steps_per_s=steps / dt,
                max_steps=eb.max_steps, rows=len(rows))


def episodes(n):
    """`n` stand-alone Experiment episodes (map ids 1 .. n) with the host policy: construction outside the clock"""
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import runner
    wall, steps = 0.0, 0
    for i in range(n):
        p = pkg.Params(debug=True, **dict(README_CFG, map_id=README_CFG['map_id'] + i))
        p.render = False
        ex = runner.Experiment(p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row = ex.run()
        torch.cuda.synchronize()
        wall += time.perf_counter() - t0
        steps += int(round(float(row[12]) / p.dt))
    return dict(leg='experiment_episodes', gaze='Owl', policy='host', episodes=n, wall_s=wall, env_steps=steps,
                s_per_episode=wall / max(n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=600, help='closed-loop leg: timed steps')
    ap.add_argument('--warmup', type=int, default=300, help='closed-loop leg: untimed steps first')
    ap.add_argument('--reps', type=int, default=3, help='closed-loop leg: timed repetitions')
    ap.add_argument('--episodes', type=int, default=0, help='stand-alone host-policy Experiment episodes to time (0: skip)')
    ap.add_argument('--workers', type=int, default=8, help='processes building the worlds')
    ap.add_argument('--no-batch', action='store_true')
    args = ap.parse_args()
    for rec in closed_loop(args.envs, args.steps, args.warmup, args.reps, args.workers):
        print(json.dumps(rec), flush=True)
    if not args.no_batch:
        batch(8, 0)                           # (first launches: code objects, allocator)
        print(json.dumps(batch(args.envs, args.workers)), flush=True)
    if args.episodes:
        print(json.dumps(episodes(args.episodes)), flush=True)


if __name__ == '__main__':
    main()
