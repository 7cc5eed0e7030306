#!/usr/bin/env python3
"""What the Jerk_Primitive planner costs on the device (include/d2d_jerk.h), everything in one call.

Per shape -- 4096 envs x 10 agents (the README world) and 512 envs x 172 agents (BASELINE config 3's agents: 50 seeded + the 122
cells of random_map_0) -- between HIP events, `--reps` times each, alternating, every run kept (not a best-of):
  step   the time per env-batch step of VecDrone2DEnv.step with planner='Jerk_Primitive' (three launches: d2d_perceive,
         d2d_jerk_plan, d2d_act)
  nomove the fused step of the NoMove planner on the same worlds (one launch; the drone does not move, so the two envs see
         different things as the steps go on: the column says what a step costs without a planner)
  plan   d2d_jerk_plan alone, launched again and again on the state the Jerk_Primitive env has reached (the tracker bookkeeping
         is idempotent on an unchanged state, so every launch does the same work)
and the mean of the primitives the reference's lazy walk tests (stat >> 8) over the envs.  An episode of these worlds lasts about a
hundred steps (the drone reaches its goal or meets an agent) and an env that is done plans on from where it ended, almost always
without a free heading -- 72 primitives, the worst case.  So `step` and `nomove` are timed in CHUNKS: reset (untimed), then
`--chunk` steps between two events, as many chunks as make the events' sum a fifth of a second or more; `plan` is timed on the
state `--chunk` / 2 steps after a reset, and `plan_worst` on the state a long run leaves (every env done).  Every record says how
many steps it timed and what the planner found there.  Every env is stepped untimed first (code objects, allocator).  The worlds
are built on the device.

Also recorded: the reference's own seconds per step from tests/golden/jerk_traces.npz (one env, on the recording machine's CPU) and
the compiler's resource report of the kernels for gfx950 (--resources-only stops after it and needs no GPU).

python tools/jerk_bench.py --out profiles/jerk_profile.json"""
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
    dict(name='readme_4096x10', envs=4096, steps=dict(step=2000, nomove=10000, plan=20000),
         params=dict(agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1)),
    dict(name='config3_512x172', envs=512, steps=dict(step=2000, nomove=6000, plan=20000),
         params=dict(agent_number=50, agent_radius=10, agent_max_speed=40, map_id=1, static_map='maps/random_map_0.npy')),
]


def resources():
    """-Rpass-analysis=kernel-resource-usage of csrc/jerk/d2d_jerk.hip for gfx950, per kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, D2D_OUT=os.path.join(tmp, 'libd2d_jerk.so'), D2D_EXTRA_FLAGS='-Rpass-analysis=kernel-resource-usage')
        r = subprocess.run(['bash', os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'jerk', 'build.sh')], env=env,
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


def timed(fn, steps, torch, env=None, chunk=None, probe=None):
    """seconds per call of fn over `steps` calls; with `env` and `chunk`: in chunks of `chunk` calls, each after an untimed reset.
    probe(): called after every chunk, its results are averaged and returned as well"""
    chunk = chunk if env is not None else steps
    total, done, seen = 0.0, 0, []
    while done < steps:
        n = min(chunk, steps - done)
        if env is not None:
            env.reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        total += t0.elapsed_time(t1) * 1e-3
        done += n
        if probe is not None:
            seen.append(probe())
    return total / steps, ([sum(x) / len(seen) for x in zip(*seen)] if seen else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--chunk', type=int, default=60, help='steps after a reset that one pair of events times')
    ap.add_argument('--scale', type=float, default=1.0, help='multiply every run\'s step count (smaller: a quicker, noisier look)')
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
    result = dict(tool='tools/jerk_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
                  resources=json.load(open(args.resources)) if args.resources else resources(), shapes=[])
    for shape in SHAPES:
        jerk = vec_env.VecDrone2DEnv(pkg.Params(planner='Jerk_Primitive', **shape['params']), shape['envs'], backend=hip, worlds='device',
                                     planner='Jerk_Primitive', device_plugins=True, gaze='NoControl')
        nomove = vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', **shape['params']), shape['envs'], backend=hip, worlds='device')
        what = dict(step=(jerk, jerk.run_step), nomove=(nomove, nomove.run_step), plan=(jerk, jerk.run_jerk_plan),
                    plan_worst=(jerk, jerk.run_jerk_plan))
        for env, fn in what.values():
            timed(fn, args.warmup, torch)

        def probe():
            return (float((jerk.jerk_stat >> 8).double().mean()), float(jerk.state.plan_ok.double().mean()),
                    float(jerk.state.flags[:, 3].double().mean()))
        runs = []
        for rep in range(args.reps):
            for name in ('step', 'nomove', 'plan', 'plan_worst'):
                env, fn = what[name]
                steps = max(1, int(shape['steps'][name.split('_')[0]] * args.scale))
                if name == 'plan':                         # the state half a chunk into an episode
                    jerk.reset()
                    timed(jerk.run_step, args.chunk // 2, torch)
                elif name == 'plan_worst':                 # the state a long run leaves
                    timed(jerk.run_step, 400, torch)
                if name in ('step', 'nomove'):
                    sec, seen = timed(fn, steps, torch, env, args.chunk, probe if name == 'step' else None)
                else:
                    sec, seen = timed(fn, steps, torch, probe=probe)
                rec = dict(rep=rep, what=name, steps=steps, chunk=args.chunk if name in ('step', 'nomove') else None, seconds_per_step=sec,
                           env_steps_per_second=shape['envs'] / sec)
                if seen:
                    rec.update(mean_primitives_tested=seen[0], plans_ok=seen[1], envs_done=seen[2])
                runs.append(rec)
                print(shape['name'], json.dumps(rec), flush=True)
        result['shapes'].append(dict(name=shape['name'], envs=shape['envs'], agents=jerk.N, params=shape['params'], S=jerk.jerk.S,
                                     unknown_tie_patterns=jerk.jerk.unknown_patterns(), runs=runs))
        del jerk, nomove
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jerk_traces.npz'))
    result['reference'] = [dict(world=str(n), agents=int(z[f'w{i}_N']), steps=int(len(z[f'w{i}_t_done'])),
                                seconds_per_step=float(z[f'w{i}_ref_seconds_per_step'])) for i, n in enumerate(z['names'])]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
