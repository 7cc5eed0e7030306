#!/usr/bin/env python3
"""What whole Jerk_Primitive episodes cost as a device batch (runner.SteppedExperimentBatch, include/d2d_gaze.h, DESIGN.md section
3.14), everything in one call.  Between HIP events, `--reps` times each, alternating, every run kept (not a best-of).

Shape: 4096 envs x 10 agents of the README world at drone_max_speed = 40, for gaze Owl and LookAhead.
  episodes    SteppedExperimentBatch.run() (its run_episodes; reading the rows is not timed) after an untimed reset: seconds, steps run, episodes per second, ms per step
  gaze, plan  d2d_gaze_act alone and d2d_jerk_plan alone, launched again and again on two states: `mid` (--mid steps into the
              episodes) and `late` (--late steps in, where most envs are done).  Repeated Owl calls walk through the policy's own
              cycle (one decision, then the held calls), which is the mix an episode sees.
  host        at 256 envs, the only path there was before this launch existed: the same step launches, the policy evaluated on the
              host each step (pull drone, target, active and kf, gaze.Owl / gaze.LookAhead per env, upload the actions), against the
              device path at 256 envs.
Also recorded: the reference's seconds per step from tests/golden/jerk_traces.npz (one env, on the recording machine's CPU) and the
compiler's resource report of the kernels for gfx950 (--resources-only stops after it and needs no GPU).

--live-ab JSON runs the other measurement and stops: run_episodes(live=True), every launch leaving finished envs alone
(include/d2d_jerk_live.h, include/d2d_rvo_live.h), against run_episodes(live=False), the loop of before, for CVM and RVO x Owl and
LookAhead at --envs envs.  Both forms in this one process, alternating, `--reps` times each, every run kept:
  whole    run_episodes() to the end after an untimed reset
  early    the first steps, one fewer than the earliest ending of that batch (taken from the whole run's own step counters): no env is
           done, so this is what the masks cost where they save nothing
  plan     d2d_jerk_plan_live and d2d_jerk_plan alone, --calls launches between one pair of events, on the state after the early steps
The summary holds the medians, the ratio of the medians and the span (max - min) of the baseline's own runs.

python tools/jerk_episodes_bench.py --out profiles/jerk_episodes.json
python tools/jerk_episodes_bench.py --reps 5 --live-ab profiles/jerk_episodes_live.json"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, map_id=1)


def resources():
    """-Rpass-analysis=kernel-resource-usage of csrc/gaze/d2d_gaze.hip for gfx950, per kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, D2D_OUT=os.path.join(tmp, 'libd2d_gaze.so'), D2D_EXTRA_FLAGS='-Rpass-analysis=kernel-resource-usage')
        r = subprocess.run(['bash', os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'gaze', 'build.sh')], env=env,
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


class _Tracker:
    def __init__(self, active, mu):
        self.active, self.mu_upds = bool(active), [mu.reshape(4, 1)]


class _Drone:
    pass


def host_policy_episodes(xb, policies, torch, np):
    """the episodes of SteppedExperimentBatch `xb` (built with gaze='external' semantics: its env's gaze launch is not used) with the
    policy objects `policies`, one per env, evaluated on the host before every step"""
    from drone2d_amd import _abi as A
    env, s = xb.env, xb.env.state
    steps = 0
    for _ in range(xb.max_steps):
        drone, target, active, kf, done = (x.cpu().numpy() for x in (s.drone, s.target, s.active, s.kf[:, :, :4], s.flags[:, A.F_DONE]))
        if done.all():
            break
        a = s.action.cpu().numpy().copy()
        for e, pol in enumerate(policies):
            if done[e]:
                continue
            d = _Drone()
            d.x, d.y, d.yaw = float(drone[e, A.D_X]), float(drone[e, A.D_Y]), float(drone[e, A.D_YAW])
            d.velocity = drone[e, A.D_VX:A.D_VY + 1].copy()
            d.trackers = [_Tracker(active[e, j], kf[e, j]) for j in range(active.shape[1])]
            a[e] = pol.plan(dict(drone=d, target=[float(target[e, 0]), float(target[e, 1])]))
        s.action.copy_(torch.from_numpy(a))
        env.gaze_state, keep = None, env.gaze_state            # the step launches alone
        try:
            env.run_episodes(max_steps=1)
        finally:
            env.gaze_state = keep
        steps += 1
    return steps


def between_events(fn, torch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3, time.perf_counter() - w, out


def live_ab(args):
    """run_episodes(live=True) against run_episodes(live=False): see the module's docstring"""
    import statistics
    import warnings
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A, _lib, runner
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    forms = (('masked', True), ('unmasked', False))
    result = dict(tool='tools/jerk_episodes_bench.py --live-ab', device=torch.cuda.get_device_name(0), reps=args.reps, envs=args.envs,
                  world=WORLD, forms={k: f'run_episodes(live={v})' for k, v in forms}, runs=[], summary=[])

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def repeat(fn, n):
        for _ in range(n):
            fn()

    for profile in ('CVM', 'RVO'):
        for g in ('Owl', 'LookAhead'):
            p = pkg.Params(planner='Jerk_Primitive', gaze_method=g, motion_profile=profile, **WORLD)
            xb = runner.SteppedExperimentBatch(p, args.envs, backend=hip, device_worlds=True)
            env = xb.env
            for _, live in forms:                           # untimed: one whole run of either form (code objects, allocator)
                env.reset()
                env.run_episodes(xb.max_steps, live=live)
            hip.sync()
            early = max(1, int(env.state.counters[:, A.C_STEPS].min()) - 1)
            rows = {}
            for rep in range(args.reps):
                for form, live in forms:
                    env.reset()
                    sec, wall, steps = between_events(lambda: env.run_episodes(xb.max_steps, live=live), torch)
                    rows[form] = xb.rows()
                    emit(dict(rep=rep, profile=profile, gaze=g, form=form, what='whole', steps=steps, seconds=sec, wall_seconds=wall,
                              ms_per_step=1e3 * sec / steps, first_ending=int(env.state.counters[:, A.C_STEPS].min())))
                for form, live in forms:
                    env.reset()
                    sec, wall, steps = between_events(lambda: env.run_episodes(early, check_every=10 ** 9, live=live), torch)
                    emit(dict(rep=rep, profile=profile, gaze=g, form=form, what='early', steps=steps, seconds=sec, wall_seconds=wall,
                              ms_per_step=1e3 * sec / steps, envs_done=int(env.state.flags[:, A.F_DONE].sum())))
                for form, fn in (('masked', lambda: hip.jerk_plan_live(env._jerk_call, env.state.flags)), ('unmasked', env.run_jerk_plan)):
                    sec, _, _ = between_events(lambda: repeat(fn, args.calls), torch)
                    emit(dict(rep=rep, profile=profile, gaze=g, form=form, what='plan', after_steps=early, calls=args.calls,
                              microseconds_per_call=1e6 * sec / args.calls))
            same = sum(all((x != x and y != y) or x == y for x, y in zip(a, b)) for a, b in zip(rows['masked'], rows['unmasked']))
            for what, key in (('whole', 'seconds'), ('early', 'ms_per_step'), ('plan', 'microseconds_per_call')):
                v = {form: [r[key] for r in result['runs'] if (r['profile'], r['gaze'], r['what'], r['form']) == (profile, g, what, form)]
                     for form, _ in forms}
                med = {form: statistics.median(x) for form, x in v.items()}
                result['summary'].append(dict(profile=profile, gaze=g, what=what, unit=key, median=med,
                                              masked_over_unmasked=med['masked'] / med['unmasked'],
                                              unmasked_span=max(v['unmasked']) - min(v['unmasked']),
                                              masked_span=max(v['masked']) - min(v['masked']),
                                              rows_equal=f'{same} of {args.envs}' if what == 'whole' else None))
                print(json.dumps(result['summary'][-1]), flush=True)
            del xb, env
    os.makedirs(os.path.dirname(os.path.abspath(args.live_ab)), exist_ok=True)
    with open(args.live_ab, 'w') as f:
        json.dump(result, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--live-ab', metavar='JSON', help='the A/B of run_episodes(live=True) against live=False alone, written there')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--host-envs', type=int, default=256)
    ap.add_argument('--mid', type=int, default=40)
    ap.add_argument('--late', type=int, default=110)
    ap.add_argument('--calls', type=int, default=2000, help='launches one pair of events times for gaze / plan alone')
    ap.add_argument('--resources', help='JSON written by --resources-only (default: compile now)')
    ap.add_argument('--resources-only', metavar='JSON', help='write the compiler\'s resource report there and stop (needs no GPU)')
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    if args.resources_only:
        with open(args.resources_only, 'w') as f:
            json.dump(resources(), f, indent=1)
        return
    if args.live_ab:
        return live_ab(args)
    import warnings
    import numpy as np
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import _abi as A, _lib, gaze, runner
    warnings.simplefilter('ignore')
    hip = _lib.HipBackend()
    result = dict(tool='tools/jerk_episodes_bench.py', device=torch.cuda.get_device_name(0), reps=args.reps, world=WORLD,
                  resources=json.load(open(args.resources)) if args.resources else resources(), runs=[])
    kinds = ('Owl', 'LookAhead')
    params = {g: pkg.Params(planner='Jerk_Primitive', gaze_method=g, **WORLD) for g in kinds}
    big = {g: runner.SteppedExperimentBatch(params[g], args.envs, backend=hip, device_worlds=True) for g in kinds}
    small = {g: runner.SteppedExperimentBatch(params[g], args.host_envs, backend=hip, device_worlds=True) for g in kinds}
    for xb in list(big.values()) + list(small.values()):      # untimed: one whole run of every shape (code objects, allocator)
        xb.env.run_episodes(xb.max_steps)
        xb.env.reset()
    hip.sync()

    def emit(rec):
        result['runs'].append(rec)
        print(json.dumps(rec), flush=True)

    def repeat(fn, n):
        for _ in range(n):
            fn()

    for rep in range(args.reps):
        for g in kinds:
            xb, env = big[g], big[g].env
            env.reset()
            sec, wall, steps = between_events(lambda: env.run_episodes(xb.max_steps), torch)     # what run() does before it reads the rows
            rows = xb.rows()
            emit(dict(rep=rep, gaze=g, what='episodes', envs=args.envs, steps=steps, seconds=sec, wall_seconds=wall,
                      episodes_per_second=args.envs / sec, ms_per_step=1e3 * sec / steps, success=sum(r[16] for r in rows),
                      mean_flight_time=float(np.mean([r[12] for r in rows]))))
            for where, steps in (('mid', args.mid), ('late', args.late)):
                env.reset()
                env.run_episodes(max_steps=steps, check_every=10 ** 9)
                done = float(env.state.flags[:, A.F_DONE].double().mean())
                for what, fn in (('gaze', env.run_gaze), ('plan', env.run_jerk_plan)):
                    sec, _, _ = between_events(lambda: repeat(fn, args.calls), torch)
                    emit(dict(rep=rep, gaze=g, what=what, where=where, after_steps=steps, envs_done=done, calls=args.calls,
                              microseconds_per_call=1e6 * sec / args.calls,
                              mean_primitives_tested=float((env.jerk_stat >> 8).double().mean())))
        for g in kinds:
            xb = small[g]
            xb.env.reset()
            sec, wall, steps = between_events(lambda: xb.env.run_episodes(xb.max_steps), torch)
            emit(dict(rep=rep, gaze=g, what='device_policy', envs=args.host_envs, steps=steps, seconds=sec, wall_seconds=wall,
                      ms_per_step=1e3 * wall / steps))
            dev_rows = xb.rows()
            xb.env.reset()
            cls = getattr(gaze, g)
            policies = [cls(xb.params) for _ in range(args.host_envs)]
            sec, wall, steps = between_events(lambda: host_policy_episodes(xb, policies, torch, np), torch)
            same = sum(a[12:15] == b[12:15] and a[16:] == b[16:] for a, b in zip(dev_rows, xb.rows()))
            emit(dict(rep=rep, gaze=g, what='host_policy', envs=args.host_envs, steps=steps, seconds=sec, wall_seconds=wall,
                      ms_per_step=1e3 * wall / max(steps, 1), rows_equal_to_device_policy=same))
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jerk_traces.npz'))
    result['reference'] = [dict(world=str(n), agents=int(z[f'w{i}_N']), steps=int(len(z[f'w{i}_t_done'])),
                                seconds_per_step=float(z[f'w{i}_ref_seconds_per_step'])) for i, n in enumerate(z['names'])]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
