#!/usr/bin/env python3
"""What whole Primitive episodes under the RVO motion profile cost as a device batch (runner.SteppedExperimentBatch,
include/d2d_stepped.h, include/d2d_rvo_live.h), everything in one call.  Between HIP events, `--reps` times
each, the variants alternating inside every repetition, every run kept (not a best-of); the summary gives the median and the spread
(max - min) of the repetitions next to it, and calls a difference below three times the larger spread "no difference".

Shape: 4096 envs x 10 agents, agent_radius 15, agent_max_speed 20, drone_max_speed 40, max_flight_time 40, for gaze LookAhead, Oxford
and Owl.
  episodes    env.run_episodes(max_steps) after an untimed reset (reading the rows is not timed): seconds, steps run, episodes per
              second, ms per step -- with the launches of include/d2d_rvo_live.h (`live`, the product) and with d2d_rvo_velocity /
              d2d_rvo_agents_step in their place (`unmasked`: finished envs keep paying for RVO and their agents keep moving, which
              no row reads), on the same env
  early       the first --early steps of the episodes, where no env is done yet, both ways: what the mask costs where it skips nothing
  launches    one more pass per gaze and variant with an event after every launch: the time per launch summed over the episode (the
              events themselves lengthen the pass; the split is for proportions)
Also recorded: the reference's seconds per step of one env on the recording host (tests/golden/primitive_rvo_episodes.npz).

python tools/primitive_rvo_episodes_bench.py --out profiles/primitive_rvo_episodes.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(planner='Primitive', motion_profile='RVO', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
             max_flight_time=40, map_id=0)
KINDS = ('LookAhead', 'Oxford', 'Owl')
VARIANTS = ('live', 'unmasked')


def between_events(fn, torch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3, time.perf_counter() - w, out


def use(env, variant):
    """the env's RVO launches of this step path: the product's, or the unmasked ones in their place"""
    if variant == 'live':
        env.__dict__.pop('_rvo_agents_live', None)
    else:
        env._rvo_agents_live = env._rvo_agents


def launches_pass(env, n, torch):
    """run_episodes(n, check_every=16) with an event after every launch -> ({launch: seconds summed over the steps}, steps)"""
    from drone2d_amd import _abi as A
    be, s, cfg = env.backend, env.state, env.cfg
    masked = '_rvo_agents_live' not in env.__dict__
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    t = 0
    torch.cuda.synchronize()
    while t < n:
        mark('start')
        if env._plan.gaze != A.GAZE_NONE:
            be.gaze_stage_live(cfg, env._st, env._plan)
        mark('gaze_stage_live')
        if masked:
            be.rvo_velocity_live(s.agents, s.agent_vel, s.pillars, s.flags, s.agent_vel_out)
            mark('rvo_velocity')
            be.rvo_agents_step_live(s.agents, s.agent_vel_out, s.flags, cfg.W_px, cfg.H_px, cfg.scale, cfg.dt)
        else:
            be.rvo_velocity(s.agents, s.agent_vel, s.pillars, s.agent_vel_out)
            mark('rvo_velocity')
            be.rvo_agents_step(s.agents, s.agent_vel_out, cfg.W_px, cfg.H_px, cfg.scale, cfg.dt)
        s.t['agent_vel'], s.t['agent_vel_out'] = s.t['agent_vel_out'], s.t['agent_vel']
        mark('rvo_agents_step')
        be.run_stages(cfg, env._st, (A.ST_PERCEIVE & ~A.ST_AGENTS) | A.ST_SKIP_DONE)
        mark('perceive')
        be.plan_stage_live(cfg, env._st, env._plan)
        mark('plan_stage_live')
        be.run_stages(cfg, env._st, A.ST_ACT | A.ST_SKIP_DONE)
        mark('act')
        t += 1
        if t % 16 == 0 and t < n and bool(s.flags[:, A.F_DONE].all()):
            break
    torch.cuda.synchronize()
    out = {}
    for (_, a), (name, b) in zip(marks, marks[1:]):
        if name != 'start':
            out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e-3
    return out, t


def summarize(runs):
    """median and spread (max - min) per (what, gaze, variant) of the figure that matters, and live against unmasked"""
    key = {'episodes': 'seconds', 'early': 'seconds'}
    groups = {}
    for r in runs:
        if r['what'] in key:
            groups.setdefault((r['what'], r['gaze'], r['variant']), []).append(r[key[r['what']]])
    out = []
    for (what, gaze, variant), v in sorted(groups.items()):
        out.append(dict(what=what, gaze=gaze, variant=variant, runs=len(v), median_seconds=statistics.median(v), spread_seconds=max(v) - min(v)))
    for what in ('episodes', 'early'):
        for gaze in KINDS:
            a, b = groups.get((what, gaze, 'live')), groups.get((what, gaze, 'unmasked'))
            if a and b:
                diff = statistics.median(b) - statistics.median(a)
                spread = max(max(a) - min(a), max(b) - min(b))
                out.append(dict(what=what + ': unmasked - live', gaze=gaze, median_difference_seconds=diff, larger_spread_seconds=spread,
                                verdict='no difference' if abs(diff) < 3 * spread else ('the mask saves' if diff > 0 else 'the mask costs'),
                                relative=diff / statistics.median(b)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--early', type=int, default=20, help='steps of the pass in which no env is done yet')
    ap.add_argument('--gaze', nargs='*', default=list(KINDS))
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A, _lib, runner
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    result = dict(tool='tools/primitive_rvo_episodes_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, envs=args.envs,
                  world=WORLD, early_steps=args.early, runs=[])
    batches = {g: runner.SteppedExperimentBatch(pkg.Params(gaze_method=g, **WORLD), args.envs, backend=hip, device_worlds=True)
               for g in args.gaze}
    for xb in batches.values():                 # untimed: one whole run of every shape and variant (code objects, allocator)
        for variant in VARIANTS:
            use(xb.env, variant)
            xb.env.run_episodes(xb.max_steps)
            xb.env.reset()
    hip.sync()

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    for rep in range(args.reps):
        for g, xb in batches.items():
            env = xb.env
            for variant in (VARIANTS if rep % 2 == 0 else VARIANTS[::-1]):
                use(env, variant)
                env.reset()
                sec, wall, steps = between_events(lambda: env.run_episodes(xb.max_steps), torch)
                rows = xb.rows()
                ends = np.array([round(r[12] / xb.params.dt) for r in rows])
                emit(dict(rep=rep, gaze=g, variant=variant, what='episodes', envs=args.envs, steps=steps, seconds=sec, wall_seconds=wall,
                          episodes_per_second=args.envs / sec, ms_per_step=1e3 * sec / steps, success=sum(r[16] for r in rows),
                          dynamic_collision=sum(r[18] for r in rows), freezing=sum(r[19] for r in rows), dead_lock=sum(r[20] for r in rows),
                          mean_steps=float(ends.mean()), median_steps=float(np.median(ends)), first_end=int(ends.min())))
                env.reset()
                sec, wall, steps = between_events(lambda: env.run_episodes(args.early, check_every=10 ** 9), torch)
                emit(dict(rep=rep, gaze=g, variant=variant, what='early', envs=args.envs, steps=steps, seconds=sec,
                          ms_per_step=1e3 * sec / steps, envs_done=int(env.state.flags[:, A.F_DONE].sum())))
    for g, xb in batches.items():
        for variant in VARIANTS:
            use(xb.env, variant)
            xb.env.reset()
            split, steps = launches_pass(xb.env, xb.max_steps, torch)
            emit(dict(gaze=g, variant=variant, what='launches', envs=args.envs, steps=steps, seconds=split,
                      microseconds_per_step={k: 1e6 * v / steps for k, v in split.items()}))
        use(xb.env, 'live')
    result['summary'] = summarize(result['runs'])
    for s in result['summary']:
        print(json.dumps(s), flush=True)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'primitive_rvo_episodes.npz'))
    result['reference'] = [dict(world=str(n), agents=int(z[f'w{i}_N']), steps=int(len(z[f'w{i}_t_done'])),
                                seconds_per_step=float(z[f'w{i}_ref_s_per_step'])) for i, n in enumerate(z['names'])]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
