#!/usr/bin/env python3
"""What the RVO motion profile costs on the device (include/d2d_rvo.h), everything in one call.

Per shape -- 4096 envs x 10 agents (the README world, NoMove) and 512 envs x 172 agents (BASELINE config 3's agents: 50 seeded +
the 122 cells of random_map_0) -- the time per env-batch step of VecDrone2DEnv.step under motion_profile='RVO' (its three launches:
d2d_rvo_velocity, d2d_rvo_agents_step, d2d_run_stages without the agents stage) alternating with the fused step of the
constant-velocity model on the same worlds, between HIP events, `--reps` times each; every run is kept, not a best-of.  A run
is as many steps as make its window a fifth of a second or more (SHAPES: `steps`; each record says how many it timed).  Both
envs are stepped untimed first (code objects, allocator).  The worlds are built on the device.  The RVO env's positions drift
from the CVM env's as the steps go on: the two do different work by design, the CVM column says what a step costs without the
decisions.

Also recorded: the reference's own seconds per step from tests/golden/rvo_traces.npz (one env, on the recording machine's CPU);
the compiler's resource report of the two kernels for gfx950 (--resources: registers, LDS, scratch; needs no GPU, and
--resources-only stops after it); and the `bench.py --gpus 1 --steps 600 --warmup 300` line of this tree and, with --parent DIR,
of a built checkout of the parent commit, alternating (libd2d_hip.so is the same in both: this only shows that nothing moved).

python tools/rvo_bench.py --out profiles/rvo_profile.json [--parent DIR]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [
    dict(name='readme_4096x10', envs=4096, steps=dict(RVO=500, CVM=10000), params=dict(agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1)),
    dict(name='config3_512x172', envs=512, steps=dict(RVO=50, CVM=6000), params=dict(agent_number=50, agent_radius=10, agent_max_speed=40, map_id=1,
                                                       static_map='maps/random_map_0.npy')),
]


def resources():
    """-Rpass-analysis=kernel-resource-usage of csrc/rvo/d2d_rvo.hip for gfx950, per kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, D2D_OUT=os.path.join(tmp, 'libd2d_rvo.so'), D2D_EXTRA_FLAGS='-Rpass-analysis=kernel-resource-usage')
        r = subprocess.run(['bash', os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'rvo', 'build.sh')], env=env,
                           capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(.*?):\s*(\S+)\s*\[-Rpass-analysis', line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == 'Function Name':
            cur = out.setdefault(re.sub(r'^_ZN\d+_GLOBAL__N_1\d+|E[A-Za-z0-9_]*$', '', val), {})
        elif cur is not None:
            cur[key] = int(val) if val.lstrip('-').isdigit() else val
    return out


def time_steps(env, steps, torch):
    a = torch.zeros(env.num_envs, dtype=torch.float64, device=env.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        env.state.action.copy_(a)
        env.run_step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / steps


def bench_line(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '600', '--warmup', '300'], cwd=tree,
                       capture_output=True, text=True, check=True)
    return json.loads([line for line in r.stdout.splitlines() if line.startswith('{')][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its bench.py line is recorded next to this tree\'s')
    ap.add_argument('--no-bench', action='store_true', help='skip the bench.py lines')
    ap.add_argument('--resources', help='JSON written by --resources-only (default: compile now)')
    ap.add_argument('--resources-only', metavar='JSON', help='write the compiler\'s resource report there and stop (needs no GPU)')
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    if args.resources_only:
        with open(args.resources_only, 'w') as f:
            json.dump(resources(), f, indent=1)
        return
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _lib, vec_env
    hip = _lib.HipBackend()
    result = dict(tool='tools/rvo_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                  resources=json.load(open(args.resources)) if args.resources else resources(), shapes=[])
    for shape in SHAPES:
        envs = {prof: vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', motion_profile=prof, **shape['params']), shape['envs'], backend=hip,
                                            worlds='device') for prof in ('RVO', 'CVM')}
        for env in envs.values():
            time_steps(env, args.warmup, torch)
        runs = []
        for rep in range(args.reps):
            for prof in ('RVO', 'CVM'):
                rec = dict(rep=rep, motion_profile=prof, steps=shape['steps'][prof], seconds_per_step=time_steps(envs[prof], shape['steps'][prof], torch))
                rec['env_steps_per_second'] = shape['envs'] / rec['seconds_per_step']
                runs.append(rec)
                print(shape['name'], json.dumps(rec), flush=True)
        vel = envs['RVO'].state.agent_vel
        assert bool(torch.isfinite(vel).all())
        result['shapes'].append(dict(name=shape['name'], envs=shape['envs'], agents=envs['RVO'].N, params=shape['params'], runs=runs))
        del envs
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rvo_traces.npz'))
    result['reference'] = [dict(world=str(n), agents=int(z[f'w{i}_agent_pos'].shape[0]), pillars=int(z[f'w{i}_obstacles'].shape[0]),
                                seconds_per_step=float(z[f'w{i}_ref_seconds_per_step'])) for i, n in enumerate(z['names'])]
    result['reference'].append(dict(world='primitive_lookahead_episode', agents=20, pillars=0, seconds_per_step=float(z['ep_ref_seconds_per_step'])))
    if not args.no_bench:
        lines = []
        for rep in range(2 if args.parent else 1):
            for which, tree in (('parent', args.parent), ('tree', ROOT)):
                if tree:
                    line = bench_line(os.path.abspath(tree))
                    lines.append(dict(which=which, rep=rep, line=line))
                    print(which, json.dumps(line)[:300], flush=True)
        result['bench'] = lines
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
