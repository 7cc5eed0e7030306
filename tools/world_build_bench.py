#!/usr/bin/env python3
"""Wall-clock cost of building the seeded worlds of a batch and making them resident, three ways:

  host0    vec_env.build_worlds(workers=0) + VecDrone2DEnv(worlds=...): the host path, one process
  host8    the same with workers=8 forked processes: the yardstick
  device   VecDrone2DEnv(worlds='device'): include/d2d_worlds.h, one launch

Shapes: BASELINE config 2 (10 agents), config 3's world (50 agents + random_map_0's 122), config 4's world (10 + obstacle_map's
14) and config 5's geometry (100 agents, 640 x 640 cells, tiled).  The host legs may build fewer worlds than the device leg
(--host-worlds); every leg reports seconds per world.

A repetition of a shape is one child process that runs the three legs one after the other, so the legs alternate over the
--reps repetitions.  The host constructions run first, before the child touches the GPU (the pool forks); then the GPU is
initialised and one small batch of either kind is built untimed (code objects, allocator); then every leg's resident part is timed
with a device synchronise on both sides.  A host leg's time is its construction plus its resident part.

python tools/world_build_bench.py --out profiles/device_worlds.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (device worlds, host worlds, Params overrides)
    'config2': (4096, 4096, dict(agent_number=10, agent_radius=15, agent_max_speed=20)),
    'config3': (4096, 1024, dict(agent_number=50, agent_radius=10, agent_max_speed=40, static_map='maps/random_map_0.npy')),
    'config4': (4096, 4096, dict(agent_number=10, agent_radius=15, agent_max_speed=20, static_map='maps/obstacle_map.npy')),
    'config5': (512, 128, dict(agent_number=100, agent_radius=15, agent_max_speed=40, map_size=[6400, 6400], init_pos=[3200, 3200],
                               target_list=[[6000, 6000]])),
}


def child(shape, n_dev, n_host):
    import drone2d_amd as pkg
    from drone2d_amd import vec_env
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', map_id=1, **SHAPES[shape][2])
    t0 = time.perf_counter()
    w8 = vec_env.build_worlds(p, n_host, workers=8)
    t1 = time.perf_counter()
    w0 = vec_env.build_worlds(p, n_host, workers=0)
    t2 = time.perf_counter()
    import torch
    vec_env.VecDrone2DEnv(p, 8, worlds=w0[:8])
    vec_env.VecDrone2DEnv(p, 8, worlds='device')

    def resident(n, worlds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        env = vec_env.VecDrone2DEnv(p, n, worlds=worlds)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        del env
        return dt
    r8, r0, rd = resident(n_host, w8), resident(n_host, w0), resident(n_dev, 'device')
    # the construction launch alone (uploads of the per-env rows, kernel, read-back of status and tracker radii) into a resident batch
    env = vec_env.VecDrone2DEnv(p, n_dev, worlds='device')
    inp = vec_env.world_inputs([p], map_ids=[p.map_id + i for i in range(n_dev)])
    torch.cuda.synchronize()
    t = time.perf_counter()
    vec_env._build_into(env.backend, inp, env.state)
    torch.cuda.synchronize()
    launch = time.perf_counter() - t
    for leg, n, build, res in (('host0', n_host, t2 - t1, r0), ('host8', n_host, t1 - t0, r8), ('device', n_dev, 0.0, rd)):
        print(json.dumps(dict(shape=shape, leg=leg, worlds=n, build_s=build, resident_s=res, total_s=build + res,
                              s_per_world=(build + res) / n, **(dict(launch_s=launch) if leg == 'device' else {}))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--worlds', type=int, default=0, help='device worlds per shape (default: the shape\'s own)')
    ap.add_argument('--host-worlds', type=int, default=0, help='host worlds per shape (default: the shape\'s own)')
    ap.add_argument('--out', help='write the summary here (JSON)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.worlds, args.host_worlds)
        return
    recs = []
    for rep in range(args.reps):
        for shape in args.shapes:
            n_dev = args.worlds or SHAPES[shape][0]
            n_host = min(args.host_worlds or SHAPES[shape][1], n_dev)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', shape, '--worlds', str(n_dev),
                                  '--host-worlds', str(n_host)], check=True, stdout=subprocess.PIPE, text=True).stdout
            for line in out.splitlines():
                if line.startswith('{'):
                    rec = dict(json.loads(line), rep=rep)
                    recs.append(rec)
                    print(json.dumps(rec), flush=True)
    summary = {}
    for shape in args.shapes:
        per = {leg: sorted(r['s_per_world'] for r in recs if r['shape'] == shape and r['leg'] == leg) for leg in ('host0', 'host8', 'device')}
        med = {leg: v[len(v) // 2] for leg, v in per.items()}
        spread8 = per['host8'][-1] - per['host8'][0]
        summary[shape] = dict(
            worlds={leg: next(r['worlds'] for r in recs if r['shape'] == shape and r['leg'] == leg) for leg in per},
            ms_per_world={leg: [1e3 * x for x in v] for leg, v in per.items()},
            median_ms_per_world={leg: 1e3 * x for leg, x in med.items()},
            host8_spread_ms_per_world=1e3 * spread8,
            device_faster_than_host8_by_more_than_its_spread=bool(med['host8'] - med['device'] > spread8),
            speedup_over_host8=med['host8'] / med['device'],
            device_launch_ms=sorted(1e3 * r['launch_s'] for r in recs if r['shape'] == shape and r['leg'] == 'device'))
    result = dict(tool='tools/world_build_bench.py', reps=args.reps, shapes=summary, runs=recs)
    print(json.dumps(dict(summary=summary)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
