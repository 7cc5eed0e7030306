#!/usr/bin/env python3
"""Wall-clock cost of the LookAhead gaze policy (main.py:10's default method) with and without the device gaze stage.

  ExperimentBatch  the experiment_rows r1 cfg (LookAhead + Primitive, tests/golden) over --envs map ids, one frozen episode each:
                   --path host   the host loop (per step: pull velocity + yaw, a Python pass over the envs, upload, one launch)
                   --path device the device gaze stage (one closed_loop call for the whole sweep)
  closed loop      env-steps/s of VecDrone2DEnv(..., gaze='LookAhead').closed_loop(--steps, auto_reset=True) (device only)

Times are wall clock around the call with a device synchronise before and after; worlds are built before the clock starts.
python tools/heading_gaze_bench.py --path both --envs 4096"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R1_CFG = dict(gaze_method='LookAhead', planner='Primitive', agent_number=30, agent_max_speed=40, agent_radius=10,
              drone_max_speed=40, map_id=0)   # tests/golden/experiment_rows.npz r1_cfg


def batch(path, envs, workers):
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import runner
    p = pkg.Params(debug=True, **R1_CFG)
    p.render = False
    eb = runner.ExperimentBatch(p, envs, workers=workers, device_gaze=(path == 'device'))
    assert eb._host_lookahead == (path == 'host')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = eb.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = int(eb.env.state.counters[:, pkg._abi.C_STEPS].sum())
    return dict(leg='experiment_batch', path=path, envs=envs, wall_s=dt, env_steps=steps, env_steps_per_s=steps / dt,
                max_steps=eb.max_steps, rows=len(rows))


def closed_loop(envs, steps, warmup, workers):
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import vec_env
    p = pkg.Params(**R1_CFG)
    worlds = vec_env.build_worlds(p, envs, workers=workers)
    env = vec_env.VecDrone2DEnv(p, envs, planner='Primitive', device_plugins=True, gaze='LookAhead', worlds=worlds)
    env.closed_loop(warmup, auto_reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env.closed_loop(steps, auto_reset=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(leg='closed_loop', gaze='LookAhead', envs=envs, steps=steps, warmup=warmup, wall_s=dt,
                env_steps_per_s=envs * steps / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--path', choices=['host', 'device', 'both'], default='both', help='ExperimentBatch gaze path')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=300, help='closed-loop leg: timed steps')
    ap.add_argument('--warmup', type=int, default=60, help='closed-loop leg: untimed steps first')
    ap.add_argument('--workers', type=int, default=8, help='processes building the worlds')
    ap.add_argument('--no-closed-loop', action='store_true')
    args = ap.parse_args()
    for path in (['host', 'device'] if args.path == 'both' else [args.path]):
        batch(path, 8, 0)                     # (first launches: code objects, allocator)
        print(json.dumps(batch(path, args.envs, args.workers)), flush=True)
    if not args.no_closed_loop:
        print(json.dumps(closed_loop(args.envs, args.steps, args.warmup, args.workers)), flush=True)


if __name__ == '__main__':
    main()
