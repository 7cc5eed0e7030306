#!/usr/bin/env python3
"""What obs['track_map'] (VecDrone2DEnv(..., tracks_obs=True), include/d2d_tracks.h) costs a learner on an
action stream.  Per cell (Primitive-CVM, Jerk-CVM) two streams live in one process and take turns, run for run, so that both see the
same clocks and the same neighbours:

  off    tracks_obs=False: the stream of before
  on     tracks_obs=True: the same step, d2d_tracks_update behind it and the copy of the window into the float32 observation

Shape: --slots 4096, 10 agents (BASELINE config 2's parameters), gaze='external', the constant action 0, --warmup steps each, then
--reps times (off, on) runs of --steps steps each between HIP events; a turn every 4 steps, as the stream's default has it.  Episodes
end and slots refill inside the runs, as they do for a learner.  Reported per cell and variant: every run, the median and the spread
(max - min) of ms per step.  The launch alone is timed too, with `force` so that every env is due: --launches calls of
d2d_tracks_update on the `on` stream's env as the last run left it, and the same with the copy.

--root DIR --variants off measures another tree (the parent commit's, which has no tracks_obs keyword) with the same loop;
--merge A.json B.json ... adds such files to --out as `parent_runs` and says whether the parent's figure and this tree's `off` figure
lie within each other's run-to-run spread.

python tools/tracks_obs_bench.py --out profiles/tracks_obs.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, max_flight_time=40, map_id=0)
CELLS = {'Primitive-CVM': dict(BASE, planner='Primitive'), 'Jerk-CVM': dict(BASE, planner='Jerk_Primitive')}


def summary(ms):
    ms = sorted(ms)
    return dict(median_ms_a_step=ms[len(ms) // 2], spread_ms_a_step=ms[-1] - ms[0], runs_ms_a_step=ms)


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _lib, vec_env
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    variants = args.variants.split(',')
    act = torch.zeros(args.slots, dtype=torch.float64, device=hip.device)
    cells = {}
    for cell, world in CELLS.items():
        streams = {}
        for variant in variants:
            kw = dict(tracks_obs=True) if variant == 'on' else {}
            env = vec_env.VecDrone2DEnv(pkg.Params(**world), args.slots, backend=hip, planner=world['planner'], device_plugins=True,
                                        gaze='external', worlds='device', **kw)
            streams[variant] = env.action_stream(refill_every=4)
        for stream in streams.values():
            for _ in range(args.warmup):
                stream.step(act)
        hip.sync()
        runs = {v: [] for v in variants}
        for rep in range(args.reps):
            for variant, stream in streams.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    obs = stream.step(act)[0]
                b.record()
                hip.sync()
                runs[variant].append(a.elapsed_time(b) / args.steps)
        out = {v: dict(summary(runs[v]), finished=streams[v].finished_now()) for v in variants}
        out['channels'] = sorted(obs)
        if 'on' in variants and 'off' in variants:
            out['on_over_off'] = out['on']['median_ms_a_step'] / out['off']['median_ms_a_step']
            out['added_ms_a_step'] = out['on']['median_ms_a_step'] - out['off']['median_ms_a_step']
        if 'on' in variants:                   # the launch alone, every env due
            env = streams['on'].env
            env._tracks.force = 1
            alone = {}
            for name, fn in (('launch', lambda: hip.tracks_update(env.cfg, env._st, env._tracks)), ('launch_and_copy', env._tracks_update)):
                for _ in range(10):
                    fn()
                hip.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    fn()
                b.record()
                hip.sync()
                alone[name + '_microseconds'] = a.elapsed_time(b) * 1e3 / args.launches
            env._tracks.force = 0
            alone.update(launches=args.launches, envs_with_an_active_tracker=int(env.state.active.bool().any(dim=1).sum()),
                         active_trackers=int(env.state.active.sum()), nonzero_cells=int(env.track_cells.sum()))
            out['launch_alone'] = alone
        for stream in streams.values():
            stream.close()
        cells[cell] = out
    return dict(tool='tools/tracks_obs_bench.py', root=os.path.basename(os.path.abspath(args.root)), device=torch.cuda.get_device_name(0),
                slots=args.slots, steps=args.steps, warmup=args.warmup, reps=args.reps, worlds=CELLS, cells=cells)


def merge(out, paths):
    """the parent tree's runs next to this tree's `off` runs: equal within the run-to-run spread?"""
    parents = [json.load(open(p)) for p in paths]
    out['parent_runs'] = [dict(root=p['root'], cells={c: p['cells'][c]['off'] for c in p['cells']}) for p in parents]
    verdict = {}
    for cell, rec in out['cells'].items():
        off = rec['off']['runs_ms_a_step']
        par = [ms for p in parents for ms in p['cells'][cell]['off']['runs_ms_a_step']]
        spread = max(max(off) - min(off), max(par) - min(par))
        diff = abs(sorted(off)[len(off) // 2] - sorted(par)[len(par) // 2])
        verdict[cell] = dict(off_median_ms=sorted(off)[len(off) // 2], parent_median_ms=sorted(par)[len(par) // 2], difference_ms=diff,
                             run_to_run_spread_ms=spread, within_the_spread=bool(diff <= spread))
    out['off_against_the_parent_commit'] = verdict
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--variants', default='off,on')
    ap.add_argument('--merge', nargs='*', default=[])
    ap.add_argument('--base', help='a file this tool wrote for this tree: merge into it instead of measuring again')
    ap.add_argument('--out')
    args = ap.parse_args()
    out = json.load(open(args.base)) if args.base else measure(args)
    if args.merge:
        out = merge(out, args.merge)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
