#!/usr/bin/env python3
"""What one cell of the reference's validation study costs as a stream over a table of episodes (runner.EpisodeStream(episodes=...),
include/d2d_worlds_table.h), and what the redraw added to the world build costs where it is off.  `--reps`
times each, the variants rotating inside every repetition, every run kept (not a best-of); the summary gives the median and the spread
(max - min) next to it, and calls a difference below three times the larger spread "no difference".

  cell      one validation_speed cell: 360 episodes (5 maps x 72 (start, target) pairs), Primitive / Oxford, 10 agents of radius 15,
            drone_max_speed 40, every world redrawn.
              stream/64, stream/360   EpisodeStream(episodes=table) over 64 and over 360 slots (refill_every 64)
              batch                   ONE 360-env batch of the same worlds built on the host (build_worlds_of(..., redraw=True),
                                      one process), run by the persistent closed loop with freeze_done
            wall seconds from before the construction to after the last row is on the host; the rows of every variant are compared
            with the first batch's.
  build     d2d_worlds_build for 4096 config-2 worlds (10 agents, radius 15, speed 20) into a resident batch, between HIP events:
              this/off    this tree's library, D2D_WE_REDRAW 0
              this/on     this tree's library, D2D_WE_REDRAW 1
              parent/off  `--parent-lib`: a libd2d_worlds.so built from a checkout of the parent commit (git worktree add DIR HEAD~1;
                          D2D_OUT=<path> DIR/gym-drone2d-activeperception_amd/csrc/worlds/build.sh), loaded next to this tree's in
                          the same process, so both are measured in the same call.  Without it the leg is left out and the JSON says so.

python tools/episode_table_bench.py --parent-lib build/parent/libd2d_worlds.so --out profiles/episode_table.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL = (10, 15, 40, 'Primitive', 'Oxford')
BUILD_WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, planner='Primitive', gaze_method='Oxford', map_id=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slots', type=int, nargs='+', default=[64, 360])
    ap.add_argument('--build-worlds', type=int, default=4096)
    ap.add_argument('--build-launches', type=int, default=20, help='launches between the two events of one build measurement')
    ap.add_argument('--parent-lib', help="libd2d_worlds.so built from a checkout of the parent commit")
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import ctypes as C
    import warnings
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _lib, runner, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    study = runner.ValidationStudy('speed')
    cell, p, table = next(c for c in study.cells() if c[0] == CELL)
    result = dict(tool='tools/episode_table_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, cell=list(cell),
                  episodes=len(table), build_worlds=args.build_worlds, build_launches=args.build_launches,
                  parent_lib=bool(args.parent_lib), runs=[])

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def stream(slots, episodes=table):
        hip.sync()
        t0 = time.perf_counter()
        xs = runner.EpisodeStream(p, episodes=episodes, slots=slots, backend=hip, redraw_agents=True, agent_speed=-1)
        rows = xs.run(refill_every=64)
        return dict(seconds=time.perf_counter() - t0, steps=xs.steps_run), rows

    def batch(episodes=table):
        hip.sync()
        t0 = time.perf_counter()
        q = runner.ExperimentBatch.accepted(p, hip)[0]
        worlds = vec_env.build_worlds_of(episodes, redraw=True)
        t1 = time.perf_counter()
        env = vec_env.VecDrone2DEnv(q, len(episodes), backend=hip, planner=q.planner, worlds=worlds, device_plugins=True, gaze=q.gaze_method)
        steps = int(np.ceil(q.max_flight_time / q.dt)) + 1
        env.closed_loop(steps, freeze_done=True)
        env.sync()
        rec = runner.batch_records(env)
        rows = [runner.study_row(pkg.with_defaults(e), rec[k], -1) for k, e in enumerate(episodes)]
        return dict(seconds=time.perf_counter() - t0, host_build_seconds=t1 - t0, steps=steps), rows

    # ---- the world build: this tree's library and the parent's, loaded side by side
    n = args.build_worlds
    bp = pkg.Params(**BUILD_WORLD)
    env = vec_env.VecDrone2DEnv(bp, n, backend=hip, worlds='device')
    libs = {'this': hip.wfn}
    if args.parent_lib:
        libs['parent'] = _lib.load_worlds_library(os.path.abspath(args.parent_lib))[1]
    specs = {}
    for redraw in (False, True):
        inp = vec_env.world_inputs([bp], map_ids=[bp.map_id + i for i in range(n)], redraw=redraw)
        up = {k: torch.from_numpy(inp[k].view('int32') if k == 'map_id' else inp[k]).to(env.device) for k in ('unit', 'cells', 'map_id', 'env_par', 'env_tgt')}
        up['tracker_radius'] = torch.zeros((n, inp['N']), dtype=torch.float64, device=env.device)
        up['obstacles'] = torch.zeros((n, inp['P'], 3), dtype=torch.int32, device=env.device)
        up['status'] = torch.zeros(n, dtype=torch.int32, device=env.device)
        specs[redraw] = (vec_env.world_spec(inp, env.cfg.grid_tile, lambda k: up[k].data_ptr() if up[k].numel() else env.state._dummy.data_ptr()), up)
    st = env.state.struct()

    def build(lib, redraw):
        spec = specs[redraw][0]
        fn = libs[lib]['build']
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        hip.sync()
        a.record()
        for _ in range(args.build_launches):
            rc = fn(C.byref(spec), C.byref(st), stream_)
            assert rc == 0, rc
        b.record()
        hip.sync()
        assert not int(specs[redraw][1]['status'].any())
        return dict(seconds=a.elapsed_time(b) * 1e-3 / args.build_launches)

    # untimed: every shape once at a small size (code objects, allocator)
    stream(4, table[:8]), batch(table[:8])
    for lib in libs:
        build(lib, False)
    build('this', True)
    reference = batch()[1]                       # untimed: the rows every timed variant is compared with

    cell_variants = [f'stream/{s}' for s in args.slots] + ['batch']
    build_variants = [(lib, False) for lib in libs] + [('this', True)]
    for rep in range(args.reps):
        k = rep % len(cell_variants)
        for v in cell_variants[k:] + cell_variants[:k]:
            rec, rows = batch() if v == 'batch' else stream(int(v.split('/')[1]))
            ref = reference
            same = len(rows) == len(ref) and all(all((a != a and b != b) or a == b for a, b in zip(x, y)) for x, y in zip(rows, ref))
            emit(dict(rec, rep=rep, what='cell', variant=v, episodes_per_second=len(table) / rec['seconds'], rows_equal_first_batch=same,
                      success=sum(r[16] for r in rows), dynamic_collision=sum(r[18] for r in rows)))
        k = rep % len(build_variants)
        for lib, redraw in build_variants[k:] + build_variants[:k]:
            emit(dict(build(lib, redraw), rep=rep, what='build', variant=f'{lib}/{"on" if redraw else "off"}'))
    groups = {}
    for r in result['runs']:
        groups.setdefault((r['what'], r['variant']), []).append(r)
    summary = []
    for (what, variant), rs in sorted(groups.items()):
        v = [r['seconds'] for r in rs]
        s = dict(what=what, variant=variant, runs=len(v), median_seconds=statistics.median(v), spread_seconds=max(v) - min(v))
        if what == 'cell':
            s.update(steps=rs[0]['steps'], rows_equal_first_batch=all(r['rows_equal_first_batch'] for r in rs))
        summary.append(s)
    med = {(s['what'], s['variant']): s for s in summary}

    def compare(what, a, b, label):
        x, y = med[(what, a)], med[(what, b)]
        diff, spread = x['median_seconds'] - y['median_seconds'], max(x['spread_seconds'], y['spread_seconds'])
        summary.append(dict(what=f'{what}: {a} - {b}', median_difference_seconds=diff, larger_spread_seconds=spread,
                            relative=diff / y['median_seconds'],
                            verdict='no difference' if abs(diff) < 3 * spread else f'{a} is {"slower" if diff > 0 else "faster"}', note=label))
    for s in args.slots:
        compare('cell', f'stream/{s}', 'batch', 'a 360-episode cell: the table stream against one host-built batch')
    if 'parent' in libs:
        compare('build', 'this/off', 'parent/off', 'd2d_worlds_build with the redraw off against the parent commit\'s build')
        p_ = med[('build', 'parent/off')]
        summary.append(dict(what='build: this/off within the parent\'s own spread',
                            value=bool(abs(med[('build', 'this/off')]['median_seconds'] - p_['median_seconds']) <= p_['spread_seconds'])))
    compare('build', 'this/on', 'this/off', 'what the redraw itself costs a build')
    result['summary'] = summary
    for s in summary:
        print(json.dumps(s), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
