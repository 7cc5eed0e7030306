#!/usr/bin/env python3
"""What streaming seeded episodes through resident slots (runner.EpisodeStream, include/d2d_worlds_stream.h)
costs against the batches that were the only way before it, everything in one call.  `--reps` times each, the variants rotating
inside every repetition, every run kept (not a best-of); the summary gives the median and the spread (max - min) next to it, and calls
a difference below three times the larger spread "no difference".

Shape: 32 768 episodes (map ids 0 ..), 10 agents, agent_radius 15, agent_max_speed 20, drone_max_speed 40, max_flight_time 40, for
Jerk_Primitive / Owl / CVM and Primitive / LookAhead / CVM.
  batches     eight consecutive 4096-env runs of the cell's batch runner (device worlds), each constructed, run and read
  stream      one EpisodeStream over 4096 slots, at refill_every 4, 16 and 64
              both: wall seconds from before the construction to after the last row is on the host (what a table of 32 768 episodes
              costs), the part of it between the first step and the last (`run_seconds`), steps, and the slot occupancy -- the
              fraction of slots that hold a live episode per step, averaged over the run: sum of the episodes' lengths /
              (slots x steps run)
  refill      per stream run, between HIP events: the time from the end of a chunk of steps to the start of the next -- harvest,
              assign, the 8-byte read, and where something finished the masked build and the resets -- summed, and per refill
  early       the first --early steps, where no slot is done: the stream env's loop against the batch runner's on fresh envs of 4096,
              and one refill there (harvest + assign + the read: everything else is skipped when nothing finished)

python tools/episode_stream_bench.py --out profiles/episode_stream.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)
CASES = {'Jerk_Primitive/Owl/CVM': dict(planner='Jerk_Primitive', gaze_method='Owl'),
         'Primitive/LookAhead/CVM': dict(planner='Primitive', gaze_method='LookAhead')}
EVERY = (4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--episodes', type=int, default=32768)
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--early', type=int, default=20)
    ap.add_argument('--cases', nargs='*', default=list(CASES))
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import warnings
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _lib, runner
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    M, B = args.episodes, args.slots
    result = dict(tool='tools/episode_stream_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, episodes=M, slots=B,
                  world=WORLD, early_steps=args.early, runs=[])

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def params(case, map_id=0):
        return pkg.Params(**dict(dict(WORLD, **CASES[case]), map_id=map_id))

    def batch_of(case, map_id, n):
        p = params(case, map_id)
        cls = runner.SteppedExperimentBatch if p.planner == 'Jerk_Primitive' else runner.ExperimentBatch
        return cls(p, n, backend=hip, device_worlds=True)

    def ends_of(rows, dt):
        return np.array([round(r[12] / dt) for r in rows])

    def batches(case):
        hip.sync()
        w0, run, steps, live, rows = time.perf_counter(), 0.0, 0, 0, []
        for k in range(-(-M // B)):
            n = min(B, M - k * B)
            xb = batch_of(case, k * B, n)
            hip.sync()
            r0 = time.perf_counter()
            got = xb.run()
            run += time.perf_counter() - r0
            took = xb.steps_run if hasattr(xb, 'steps_run') else xb.max_steps
            steps += took
            live += int(ends_of(got, xb.params.dt).sum())
            rows += got
            slots_steps = B * steps
            del xb
        return dict(seconds=time.perf_counter() - w0, run_seconds=run, steps=steps, occupancy=live / slots_steps), rows

    def stream(case, every):
        hip.sync()
        w0 = time.perf_counter()
        xs = runner.EpisodeStream(params(case), M, B, backend=hip)
        env, marks = xs.env, []
        inner = env._episode_steps

        def steps(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inner(n)
            b.record()
            marks.append((a, b))
        env._episode_steps = steps
        hip.sync()
        r0 = time.perf_counter()
        rows = xs.run(refill_every=every)
        run = time.perf_counter() - r0
        sec = time.perf_counter() - w0
        gaps = [x[1].elapsed_time(y[0]) * 1e-3 for x, y in zip(marks, marks[1:])]
        live = int(ends_of(rows, xs.params.dt).sum())
        return dict(seconds=sec, run_seconds=run, steps=xs.steps_run, occupancy=live / (B * xs.steps_run), refills=len(gaps),
                    refill_seconds=sum(gaps), refill_microseconds_each=1e6 * sum(gaps) / max(len(gaps), 1),
                    build_failed=len(xs.build_failed)), rows

    def early(case, which):
        """the first args.early steps of fresh envs: seconds between events"""
        if which == 'stream':
            env = runner.EpisodeStream(params(case), M, B, backend=hip).env
            fn = lambda: env._episode_steps(args.early)                                     # noqa: E731
        else:
            xb = batch_of(case, 0, B)
            env = xb.env
            fn = (lambda: env.run_episodes(args.early, check_every=10 ** 9)) if env.jerk is not None else \
                (lambda: env.closed_loop(args.early, freeze_done=True))                    # noqa: E731
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record()
        fn()
        b.record()
        hip.sync()
        return dict(seconds=a.elapsed_time(b) * 1e-3, slots_done=int(env.state.flags[:, 3].sum()))

    def noop_refill(case):
        """one refill on a fresh stream env after args.early steps (nothing done): harvest, assign and the 8-byte read"""
        env = runner.EpisodeStream(params(case), M, B, backend=hip).env
        dev = env.device
        slot, refill = torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
        ids, counts = torch.zeros(B, dtype=torch.int32, device=dev), torch.tensor([B, 0], dtype=torch.int64, device=dev)
        rows = torch.full((M, 8), -1, dtype=torch.int32, device=dev)
        env._episode_steps(args.early)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record()
        hip.stream_harvest(env.cfg, env._st, slot, rows)
        hip.stream_assign(env.state.flags, M, 0, slot, ids, refill, counts)
        finished = int(counts[1])
        b.record()
        hip.sync()
        return dict(seconds=a.elapsed_time(b) * 1e-3, finished=finished)

    variants = ['batches'] + [f'stream/{r}' for r in EVERY]
    for case in args.cases:                       # untimed: every shape once at a small size (code objects, allocator, the tie table)
        M, B = 64, 16
        batches(case), [stream(case, r) for r in EVERY]
        M, B = args.episodes, args.slots
    reference = {}
    for rep in range(args.reps):
        for case in args.cases:
            order = variants[rep % len(variants):] + variants[:rep % len(variants)]
            for v in order:
                rec, rows = batches(case) if v == 'batches' else stream(case, int(v.split('/')[1]))
                if v == 'batches' and case not in reference:
                    reference[case] = rows
                same = len(rows) == len(reference.get(case, rows)) and all(
                    all((a != a and b != b) or a == b for a, b in zip(x, y)) for x, y in zip(rows, reference.get(case, rows)))
                emit(dict(rec, rep=rep, case=case, variant=v, what='episodes', episodes_per_second=M / rec['seconds'],
                          rows_equal_first_batches=same, success=sum(r[16] for r in rows), mean_steps=float(np.mean([r[12] for r in rows]) / 0.1)))
            for which in (('stream', 'batch') if rep % 2 == 0 else ('batch', 'stream')):
                emit(dict(early(case, which), rep=rep, case=case, variant=which, what='early', steps=args.early))
            emit(dict(noop_refill(case), rep=rep, case=case, variant='stream', what='noop_refill'))
    groups = {}
    for r in result['runs']:
        groups.setdefault((r['what'], r['case'], r['variant']), []).append(r)
    summary = []
    for (what, case, variant), rs in sorted(groups.items()):
        v = [r['seconds'] for r in rs]
        s = dict(what=what, case=case, variant=variant, runs=len(v), median_seconds=statistics.median(v), spread_seconds=max(v) - min(v))
        if what == 'episodes':
            s.update(median_run_seconds=statistics.median(r['run_seconds'] for r in rs), occupancy=rs[0]['occupancy'], steps=rs[0]['steps'],
                     rows_equal_first_batches=all(r['rows_equal_first_batches'] for r in rs))
            if 'refills' in rs[0]:
                s.update(refills=rs[0]['refills'], median_refill_seconds=statistics.median(r['refill_seconds'] for r in rs),
                         median_refill_microseconds_each=statistics.median(r['refill_microseconds_each'] for r in rs))
        summary.append(s)
    med = {(s['what'], s['case'], s['variant']): s for s in summary}
    for case in args.cases:
        b = med[('episodes', case, 'batches')]
        for r in EVERY:
            a = med[('episodes', case, f'stream/{r}')]
            diff, spread = b['median_seconds'] - a['median_seconds'], max(a['spread_seconds'], b['spread_seconds'])
            summary.append(dict(what='episodes: batches - stream', case=case, refill_every=r, median_difference_seconds=diff,
                                larger_spread_seconds=spread, relative=diff / b['median_seconds'],
                                verdict='no difference' if abs(diff) < 3 * spread else ('the stream is faster' if diff > 0 else 'the stream is slower')))
        a, b = med[('early', case, 'stream')], med[('early', case, 'batch')]
        diff, spread = a['median_seconds'] - b['median_seconds'], max(a['spread_seconds'], b['spread_seconds'])
        summary.append(dict(what='early: stream - batch', case=case, median_difference_seconds=diff, larger_spread_seconds=spread,
                            verdict='no difference' if abs(diff) < 3 * spread else ('the stream env is slower' if diff > 0 else 'the stream env is faster')))
    result['summary'] = summary
    for s in summary:
        print(json.dumps(s), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
