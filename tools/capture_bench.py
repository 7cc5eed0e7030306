#!/usr/bin/env python3
"""What a capture.Capture costs a stream (include/d2d_capture.h), everything in one process.  `--reps` times each,
the variants rotating inside every repetition, every run kept (not a best-of); the summary gives the median and the spread (max - min)
and calls a difference below three times the larger spread "no difference".

Shape: 4096 slots, 10 agents, 640 x 480 px, the world of profiles/episode_stream.json and profiles/action_stream.json.  The variant
`none` is the stream without a capture, which is the parent commit's code path; `c<per_turn>/d<downsample>` carries
Capture(kinds=('static', 'dynamic'), capacity=256, per_turn, downsample).
  episodes  runner.EpisodeStream of 32768 episodes, Jerk_Primitive / Owl / CVM, refill_every 16, on the wall clock around run() (which
            ends in a synchronise): episodes a second
  step      the first --steps steps of fresh envs of an action stream with refill_every 1 (Jerk_Primitive / CVM and Primitive / CVM, the
            constant action 0): the capture's three launches are queued at every step.  Under Primitive no slot ends inside the window
            and they find nothing to do -- the empty turn, one workgroup plus per_turn x tiles workgroups that exit at once; under
            Jerk_Primitive a few slots do end and are drawn (`slots_done`, `matched` of each run and of the summary say how many).
            Between HIP events and on the wall clock
  turn      Capture.queue() alone, 20 calls a sample between HIP events, on envs 3 steps in: `empty` with no slot done, `full` with
            every slot declared done by a static collision, so that per_turn frames are drawn a call (the counts are put back to 0
            in front of every call, a device fill inside the timed window)

--root DIR --variants none measures another tree (the parent commit's, which has no capture) with the same loops in a process of its
own; --base FILE --merge A.json B.json ... adds such files to FILE's result as `parent_runs` and says, per measurement, whether the
parent's figure and this tree's `none` lie within each other's spread.  profiles/capture.json: the parent's tree measured before and
after this tree's run in the same call.

python tools/capture_bench.py --out profiles/capture.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)
STEP_CASES = {'Jerk_Primitive/CVM': dict(planner='Jerk_Primitive'), 'Primitive/CVM': dict(planner='Primitive')}


KEY = {'episodes': 'episodes_per_second', 'step': 'microseconds_a_step', 'turn': 'microseconds_each'}


def merge(out, paths):
    """the parent tree's `none` runs next to this tree's: equal within the spread?"""
    parents = [json.load(open(p)) for p in paths]
    out['parent_runs'] = [dict(root=p.get('root'), runs=p['runs']) for p in parents]
    verdict = []
    for what, case in sorted({(r['what'], r['case']) for r in out['runs'] if r['variant'] == 'none'}):
        mine = [r[KEY[what]] for r in out['runs'] if (r['what'], r['case'], r['variant']) == (what, case, 'none')]
        par = [r[KEY[what]] for p in parents for r in p['runs'] if (r['what'], r['case'], r['variant']) == (what, case, 'none')]
        if not par:
            continue
        diff, spread = statistics.median(mine) - statistics.median(par), max(max(mine) - min(mine), max(par) - min(par))
        verdict.append(dict(what=what, case=case, unit=KEY[what], none_median=statistics.median(mine), parent_median=statistics.median(par),
                            parent_runs=len(par), parent_spread=max(par) - min(par), difference=diff, larger_spread=spread,
                            within_the_spread=bool(abs(diff) <= spread)))
    out['none_against_the_parent_commit'] = verdict
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--episodes', type=int, default=32768)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--root', default=ROOT, help='the tree to measure (default: this one)')
    ap.add_argument('--variants', default='', help="comma-separated, e.g. 'none' for a tree without capture.py (default: all)")
    ap.add_argument('--merge', nargs='*', default=[], help='files this tool wrote for the parent tree')
    ap.add_argument('--base', help='a file this tool wrote for this tree: merge into it instead of measuring again')
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    result = json.load(open(args.base)) if args.base else measure(args)
    if args.merge:
        result = merge(result, args.merge)
        for v in result['none_against_the_parent_commit']:
            print(json.dumps(v), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A
    from drone2d_amd import _lib, runner, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    dev = hip.device
    result = dict(tool='tools/capture_bench.py', root=os.path.basename(os.path.abspath(args.root)), device=torch.cuda.get_device_name(0),
                  reps=args.reps, slots=args.slots, episodes=args.episodes, steps=args.steps, launches=args.launches, world=WORLD, map_px=[640, 480], runs=[])

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def variants(B):
        every = ['none'] + [f'c{n}/d{d}' for n in sorted({min(64, B), B}) for d in (1, 4)]
        return [v for v in every if not args.variants or v in args.variants.split(',')]

    def cap_of(env, v, **kw):
        if v == 'none':
            return None
        from drone2d_amd import capture
        n, d = v[1:].split('/d')
        return capture.Capture(env, per_turn=int(n), downsample=int(d), **kw)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        w0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        hip.sync()
        return dict(seconds=a.elapsed_time(b) * 1e-3, wall_seconds=time.perf_counter() - w0)

    def episodes_variant(v, B, M):
        p = pkg.Params(**dict(WORLD, planner='Jerk_Primitive', gaze_method='Owl'))
        xs = runner.EpisodeStream(p, M, B, backend=hip, **({} if v == 'none' else dict(capture=lambda env: cap_of(env, v))))
        hip.sync()
        t0 = time.perf_counter()
        xs.run(refill_every=16)
        sec = time.perf_counter() - t0
        rec = dict(seconds=sec, episodes_per_second=M / sec, steps=xs.steps_run, collisions=int(((xs.records[:, 4] == 1) | (xs.records[:, 4] == 2)).sum()))
        if getattr(xs, 'capture', None) is not None:
            rec.update(taken=xs.capture.taken(), dropped=xs.capture.dropped(), matched=xs.capture.matched())
        return rec

    def env_of(case, B):
        p = pkg.Params(**dict(WORLD, **STEP_CASES[case]))
        return vec_env.VecDrone2DEnv(p, B, backend=hip, planner=p.planner, worlds='device', device_plugins=True, gaze='external')

    def step_variant(case, v, B, n):
        env = env_of(case, B)
        cap = cap_of(env, v)
        stream = env.action_stream(4 * B, refill_every=1, **({} if cap is None else dict(capture=cap)))
        act = torch.zeros(B, dtype=torch.float64, device=dev)
        stream.step(act)                                       # (the capture's scratch and call are made by its first turn)
        rec = timed(lambda: [stream.step(act) for _ in range(n)])
        rec['slots_done'] = int(env.state.flags[:, A.F_DONE].sum())
        rec['matched'] = cap.matched() if cap is not None else 0
        stream.close()
        rec['microseconds_a_step'] = 1e6 * rec['seconds'] / n
        rec['wall_microseconds_a_step'] = 1e6 * rec['wall_seconds'] / n
        return rec

    def turn_variant(case, v, B, full):
        env = env_of(case, B)
        for _ in range(3):
            env.state.action.zero_()
            env._episode_steps(1)
        if full:
            env.state.flags[:, A.F_COLLISION] = 1
            env.state.flags[:, A.F_DONE] = 1
        cap = cap_of(env, v, capacity=int(v[1:].split('/d')[0]))
        slot = torch.arange(B, dtype=torch.int32, device=dev)
        cap.queue(slot)

        def loop():
            for _ in range(args.launches):
                cap.counts.zero_()
                cap.queue(slot)
        rec = timed(loop)
        rec['taken'] = cap.taken()
        rec['microseconds_each'] = 1e6 * rec['seconds'] / args.launches
        rec['wall_microseconds_each'] = 1e6 * rec['wall_seconds'] / args.launches
        return rec

    for v in variants(16):                       # untimed: every shape once at a small size (code objects, allocator, the tie table)
        episodes_variant(v, 16, 48)
        for case in STEP_CASES:
            step_variant(case, v, 16, 3)
            if v != 'none':
                turn_variant(case, v, 16, True)
    B = args.slots
    vs = variants(B)
    for rep in range(args.reps):
        order = vs[rep % len(vs):] + vs[:rep % len(vs)]
        for v in order:
            emit(dict(episodes_variant(v, B, args.episodes), rep=rep, case='Jerk_Primitive/Owl/CVM', variant=v, what='episodes'))
        for case in STEP_CASES:
            for v in order:
                emit(dict(step_variant(case, v, B, args.steps), rep=rep, case=case, variant=v, what='step'))
            for v in order:
                if v == 'none':
                    continue
                emit(dict(turn_variant(case, v, B, False), rep=rep, case=case, variant=v + '/empty', what='turn'))
                if int(v[1:].split('/d')[0]) <= 64:
                    emit(dict(turn_variant(case, v, B, True), rep=rep, case=case, variant=v + '/full', what='turn'))
    groups = {}
    for r in result['runs']:
        groups.setdefault((r['what'], r['case'], r['variant']), []).append(r)
    summary = []
    for (what, case, variant), rs in sorted(groups.items()):
        x = [r[KEY[what]] for r in rs]
        s = dict(what=what, case=case, variant=variant, runs=len(x), unit=KEY[what], median=statistics.median(x), spread=max(x) - min(x))
        if what != 'episodes':
            w = [r['wall_' + KEY[what]] for r in rs]
            s.update(median_wall=statistics.median(w), spread_wall=max(w) - min(w))
        if what == 'step':                     # slots that ended inside the timed steps, and frames drawn for them: 0, 0 is the empty turn alone
            s.update(slots_done=max(r['slots_done'] for r in rs), matched=max(r['matched'] for r in rs))
        summary.append(s)
    med = {(s['what'], s['case'], s['variant']): s for s in summary}
    for (what, case, variant), s in sorted(med.items()):
        if what == 'turn' or variant == 'none' or (what, case, 'none') not in med:
            continue
        base = med[(what, case, 'none')]
        for f, sp in (('median', 'spread'),) + ((('median_wall', 'spread_wall'),) if what == 'step' else ()):
            diff, larger = s[f] - base[f], max(s[sp], base[sp])
            summary.append(dict(what=f'{what}: {variant} - none', case=case, field=f, unit=KEY[what], difference=diff, larger_spread=larger,
                                relative=diff / base[f], verdict='no difference' if abs(diff) < 3 * larger else 'a difference'))
    result['summary'] = summary
    for s in summary:
        print(json.dumps(s), flush=True)
    return result


if __name__ == '__main__':
    main()
