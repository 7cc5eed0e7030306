#!/usr/bin/env python3
"""What the turn of an action stream (VecDrone2DEnv.action_stream, include/d2d_worlds_turn.h) costs, everything
in one process.  `--reps` times each, the variants rotating inside every repetition, every run kept (not a best-of); the summary gives
the median and the spread (max - min), and calls a difference below three times the larger spread "no difference".

Shape: 4096 slots, 10 agents, agent_radius 15, agent_max_speed 20, drone_max_speed 40, max_flight_time 40, the constant action 0, for
Jerk_Primitive / CVM and Primitive / CVM.
  step      the first --steps steps of fresh envs, where no slot is done, between HIP events and on the wall clock:
              action/1, /4, /16   ActionStream.step at that refill_every (the turn's launches are queued and find nothing to do)
              no_turn             the same step loop without any turn: the action write and VecDrone2DEnv._episode_steps(1), the launches
                                  run_episodes() queues, which this tree leaves as they were
              rounds/1            stream_rounds(refill_every=1) of before, on an env with gaze='NoControl' (the resident action 0, the
                                  same step launches): harvest, assign and the 8-byte read after every step
  restore   d2d_stream_restore + the masked resets against _refill_rest() for the same mask, 20 launches a sample between HIP events,
            with 1, 64 and all slots set
  harvest   d2d_stream_harvest of this tree against the one of `--parent-lib` (libd2d_worlds.so built from the parent commit, loaded
            into the same process), every slot done, 20 launches a sample

python tools/action_stream_bench.py --out profiles/action_stream.json [--parent-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)
CASES = {'Jerk_Primitive/CVM': dict(planner='Jerk_Primitive'), 'Primitive/CVM': dict(planner='Primitive')}
EVERY = (1, 4, 16)


class _Stop(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--cases', nargs='*', default=list(CASES))
    ap.add_argument('--parent-lib', help="the parent commit's libd2d_worlds.so, for the harvest comparison")
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A
    from drone2d_amd import _lib, action_stream, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    dev = hip.device
    result = dict(tool='tools/action_stream_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, slots=args.slots,
                  steps=args.steps, launches=args.launches, world=WORLD, runs=[])

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def env_of(case, B, gaze='external'):
        p = pkg.Params(**dict(WORLD, **CASES[case]))
        return vec_env.VecDrone2DEnv(p, B, backend=hip, planner=p.planner, worlds='device', device_plugins=True, gaze=gaze)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        w0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        hip.sync()
        return dict(seconds=a.elapsed_time(b) * 1e-3, wall_seconds=time.perf_counter() - w0)

    def step_variant(case, v, B, n):
        if v.startswith('action/'):
            stream = env_of(case, B).action_stream(4 * B, refill_every=int(v.split('/')[1]))
            act = torch.zeros(B, dtype=torch.float64, device=dev)
            rec = timed(lambda: [stream.step(act) for _ in range(n)])
            rec['slots_done'] = int(stream.env.state.flags[:, A.F_DONE].sum())
            stream.close()
        elif v == 'no_turn':
            env = env_of(case, B)
            act = torch.zeros(B, dtype=torch.float64, device=dev)

            def loop():
                for _ in range(n):
                    env.state.action.copy_(act)
                    env._episode_steps(1)
            rec = timed(loop)
            rec['slots_done'] = int(env.state.flags[:, A.F_DONE].sum())
        else:
            env = env_of(case, B, gaze='NoControl')
            inner, left = env._episode_steps, [n]

            def steps(k):
                if left[0] == 0:
                    raise _Stop()
                left[0] -= 1
                inner(k)
            env._episode_steps = steps

            def loop():
                try:
                    for _ in env.stream_rounds(4 * B, refill_every=1):
                        pass
                except _Stop:
                    pass
            rec = timed(loop)
            rec['slots_done'] = int(env.state.flags[:, A.F_DONE].sum())
        rec['microseconds_a_step'] = 1e6 * rec['seconds'] / n
        rec['wall_microseconds_a_step'] = 1e6 * rec['wall_seconds'] / n
        return rec

    def restore_variant(case, v, env, refill, prev, packed):
        if v == 'restore':
            def fn():
                for _ in range(args.launches):
                    hip.stream_restore(packed[0], packed[1], refill)
                    env.reset_plugins(refill)
        else:
            def fn():
                for _ in range(args.launches):
                    env._refill_rest(refill)
        rec = timed(fn)
        rec['microseconds_each'] = 1e6 * rec['seconds'] / args.launches
        rec['wall_microseconds_each'] = 1e6 * rec['wall_seconds'] / args.launches
        return rec

    parent = None
    if args.parent_lib:
        plib = C.CDLL(os.path.abspath(args.parent_lib))
        parent = A.bind_worlds_stream(plib)['stream_harvest']

    def harvest_variant(v, env, slot, rows):
        fn = hip.sfn['stream_harvest'] if v == 'this' else parent
        st, B = env._st, env.num_envs

        def loop():
            for _ in range(args.launches):
                rc = fn(C.byref(st), slot.data_ptr(), B, env.cfg.W, env.cfg.H, env.cfg.grid_tile, rows.shape[0], rows.data_ptr(), hip._stream())
                assert rc == 0
        rec = timed(loop)
        rec['microseconds_each'] = 1e6 * rec['seconds'] / args.launches
        return rec

    step_variants = [f'action/{r}' for r in EVERY] + ['no_turn', 'rounds/1']
    for case in args.cases:                      # untimed: every shape once at a small size (code objects, allocator, the tie table)
        for v in step_variants:
            step_variant(case, v, 16, 3)
    B = args.slots
    masks = {}
    for n in sorted({1, min(64, B), B}):
        m = torch.zeros(B, dtype=torch.uint8, device=dev)
        m[torch.linspace(0, B - 1, n).long().to(dev)] = 1
        masks[n] = m
    for rep in range(args.reps):
        for case in args.cases:
            order = step_variants[rep % len(step_variants):] + step_variants[:rep % len(step_variants)]
            for v in order:
                emit(dict(step_variant(case, v, B, args.steps), rep=rep, case=case, variant=v, what='step'))
            env = env_of(case, B)
            for _ in range(3):
                env.state.action.zero_()
                env._episode_steps(1)
            prev = torch.zeros(B, dtype=torch.int32, device=dev)
            packed = action_stream.pack_items(action_stream.restore_items(env, prev), dev)
            for n, refill in masks.items():
                for v in (('restore', 'refill_rest') if rep % 2 == 0 else ('refill_rest', 'restore')):
                    emit(dict(restore_variant(case, v, env, refill, prev, packed), rep=rep, case=case, variant=f'{v}/{n}', what='restore',
                              items=packed[1]))
            env.state.flags[:, A.F_DONE] = 1
            slot = torch.arange(B, dtype=torch.int32, device=dev)
            rows = torch.full((B, A.STREAM_ROW_F), -1, dtype=torch.int32, device=dev)
            for v in ((('this', 'parent') if rep % 2 == 0 else ('parent', 'this')) if parent else ('this',)):
                emit(dict(harvest_variant(v, env, slot, rows), rep=rep, case=case, variant=v, what='harvest'))
            del env
    groups = {}
    for r in result['runs']:
        groups.setdefault((r['what'], r['case'], r['variant']), []).append(r)
    summary = []
    for (what, case, variant), rs in sorted(groups.items()):
        key = 'microseconds_a_step' if what == 'step' else 'microseconds_each'
        v = [r[key] for r in rs]
        s = dict(what=what, case=case, variant=variant, runs=len(v), median_microseconds=statistics.median(v), spread_microseconds=max(v) - min(v))
        if what != 'harvest':
            w = [r['wall_' + key] for r in rs]
            s.update(median_wall_microseconds=statistics.median(w), spread_wall_microseconds=max(w) - min(w))
        if what == 'step':
            s['slots_done'] = max(r['slots_done'] for r in rs)
        summary.append(s)
    med = {(s['what'], s['case'], s['variant']): s for s in summary}

    def compare(what, case, a, b, label, field='median_microseconds', spread='spread_microseconds'):
        x, y = med[(what, case, a)], med[(what, case, b)]
        diff, sp = x[field] - y[field], max(x[spread], y[spread])
        summary.append(dict(what=f'{what}: {label}', case=case, field=field, median_difference_microseconds=diff, larger_spread_microseconds=sp,
                            relative=diff / y[field] if y[field] else None,
                            verdict='no difference' if abs(diff) < 3 * sp else (f'{a} is slower' if diff > 0 else f'{a} is faster')))

    for case in args.cases:
        for r in EVERY:
            for f, sp in (('median_microseconds', 'spread_microseconds'), ('median_wall_microseconds', 'spread_wall_microseconds')):
                compare('step', case, f'action/{r}', 'no_turn', f'action/{r} - no_turn', f, sp)
        for r in EVERY[1:]:
            compare('step', case, 'action/1', f'action/{r}', f'action/1 - action/{r}', 'median_wall_microseconds', 'spread_wall_microseconds')
        compare('step', case, 'rounds/1', 'action/1', 'rounds/1 - action/1', 'median_wall_microseconds', 'spread_wall_microseconds')
        for n in masks:
            compare('restore', case, f'restore/{n}', f'refill_rest/{n}', f'restore - refill_rest, {n} slots set')
        if parent:
            compare('harvest', case, 'this', 'parent', 'this - parent')
    result['summary'] = summary
    for s in summary:
        print(json.dumps(s), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
