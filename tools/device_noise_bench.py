#!/usr/bin/env python3
"""Wall-clock cost of drawing the measurement noise on the device (var_cam != 0, d2d_state.rng).

Closed loops of Oxford + Primitive on the device, VecDrone2DEnv(...).closed_loop(--steps, auto_reset=True), --reps timed
repetitions on one batch after --warmup untimed steps, in env-steps/s:

  --leg device   var_cam = 2, every agent in view gets its np.random.randn(2) from the env's own stream on the device
  --leg rows     var_cam = 2 with --rows pre-uploaded rows of standard normals (set_noise): the same kernels minus the generation.
                 The yardstick; it is all a library without the stream can run (D2D_LIB=<the parent's library>)
  --leg quiet    var_cam = 0: no noise at all (the specialised kernels on the default geometry)
  --leg batch    ExperimentBatch(var_cam=2) over --envs map ids, one frozen episode each, and --episodes stand-alone Experiment
                 episodes of the same settings (the env facade: per step a device-to-host copy of `hit` and numpy's draws)

--agents 10: the README configuration; --agents config3: BASELINE config 3's world (50 agents + random_map_0's 122).
Times are wall clock around the call with a device synchronise before and after; worlds are built before the clock starts.
python tools/device_noise_bench.py --leg device --envs 4096 --agents 10 --steps 600 --warmup 300 --reps 3"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLDS = {'10': dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, map_id=1),
          'config3': dict(agent_number=50, agent_radius=10, agent_max_speed=40, static_map='maps/random_map_0.npy', map_id=1)}


def closed_loop(leg, agents, envs, steps, warmup, reps, rows, distinct, workers):
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import vec_env
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', var_cam=0 if leg == 'quiet' else 2, **WORLDS[agents])
    worlds = vec_env.build_worlds(p, min(distinct, envs), workers=workers)
    env = vec_env.VecDrone2DEnv(p, envs, planner='Primitive', device_plugins=True, gaze='Oxford',
                                worlds=[worlds[i % len(worlds)] for i in range(envs)])
    if leg == 'rows':
        g = torch.Generator(device=env.device).manual_seed(1)
        env.set_noise(torch.randn((rows, envs, env.N, 2), dtype=torch.float64, device=env.device, generator=g))
    assert (leg == 'device') == (env.device_noise and env.state.noise is None)
    env.closed_loop(warmup, auto_reset=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.closed_loop(steps, auto_reset=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = dict(leg=leg, agents=env.N, envs=envs, steps=steps, warmup=warmup, wall_s=dt, env_steps_per_s=envs * steps / dt,
                   library=os.environ.get('D2D_LIB', 'tree'))
        if leg == 'device':
            r = env.state.rng.cpu().numpy().view(np.uint32)
            rec['pairs_per_env_step_since_reset'] = float(r[:, 625].sum()) / max(1, int(env.state.counters[:, 0].sum()))
        out.append(rec)
    return out


def batch(envs, episodes, workers):
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import runner
    kw = dict(gaze_method='Oxford', planner='Primitive', var_cam=2, **WORLDS['10'])
    p = pkg.Params(debug=True, **kw)
    p.render = False
    runner.ExperimentBatch(p, 8).run()                      # (first launches: code objects, allocator)
    eb = runner.ExperimentBatch(p, envs, workers=workers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = eb.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = int(eb.env.state.counters[:, pkg._abi.C_STEPS].sum())
    out = [dict(leg='experiment_batch', var_cam=2, envs=envs, wall_s=dt, env_steps=steps, env_steps_per_s=steps / dt, rows=len(rows))]
    wall, esteps = 0.0, 0
    for i in range(episodes):
        q = pkg.Params(debug=True, **dict(kw, map_id=kw['map_id'] + i))
        q.render = False
        ex = runner.Experiment(q)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row = ex.run()
        torch.cuda.synchronize()
        wall += time.perf_counter() - t0
        esteps += int(round(float(row[12]) / q.dt))
    if episodes:
        out.append(dict(leg='experiment_episodes', var_cam=2, episodes=episodes, wall_s=wall, env_steps=esteps,
                        s_per_episode=wall / episodes, extrapolated_s_for_envs=wall / episodes * envs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['device', 'rows', 'quiet', 'batch'], default='device')
    ap.add_argument('--agents', choices=sorted(WORLDS), default='10')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--warmup', type=int, default=300)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=64, help='--leg rows: noise rows uploaded (a run wraps around them)')
    ap.add_argument('--distinct-worlds', type=int, default=512, help='worlds built on the host, tiled over the batch')
    ap.add_argument('--episodes', type=int, default=8, help='--leg batch: stand-alone Experiment episodes to time')
    ap.add_argument('--workers', type=int, default=8, help='processes building the worlds')
    args = ap.parse_args()
    if args.leg == 'batch':
        recs = batch(args.envs, args.episodes, args.workers)
    else:
        recs = closed_loop(args.leg, args.agents, args.envs, args.steps, args.warmup, args.reps, args.rows, args.distinct_worlds,
                           args.workers)
    for rec in recs:
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
