#!/usr/bin/env python3
"""Recorder of tests/golden/swept_episodes.npz: the map Primitive.replan_check returns (traj_planner.py:220-233) on every step of four
whole episodes of the reference's gym-2d-perception-v2 env (envs/drone_v2.py) under --planner Primitive --gaze_method LookAhead, and
its crop around the drone as the gaze learner's env makes it (envs/training_v3.py:206-209), through make_golden.py's stubs.

Per episode (prefix e<i>_): cfg (the parameters, JSON) and per step
  action   what LookAhead answered, the action the step was taken with
  n, m     the trajectory's length as replan_check found it, and the waypoints it marked before it returned (m < n: a tracker hit)
  map      the returned map [W, H] uint8
  crop     [L, L] uint8: the map zero-padded by 2 * (depth // scale) and cut around the drone's cell after the step
The maps are sparse: savez_compressed.  What is stored is data; runs only where the reference is present.

Usage:  python tests/golden/make_swept_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

BASE = dict(gaze_method='LookAhead', drone_max_speed=40)
EPISODES = [
    dict(BASE, map_id=0, agent_number=30, agent_max_speed=40, agent_radius=10),
    dict(BASE, map_id=3, agent_number=30, agent_max_speed=40, agent_radius=10),
    dict(BASE, map_id=1, agent_number=10, agent_max_speed=20, agent_radius=15),
    dict(gaze_method='LookAhead', map_id=22, agent_number=2, agent_max_speed=10, agent_radius=8),     # the default drone_max_speed
]


def record(kw):
    p = G.make_params(planner='Primitive', **kw)
    env = G.Drone2DEnv2(p)
    pol = getattr(G.yaw_planner, p.gaze_method)
    pol.__init__(pol, p)
    planner = env.planner
    seen = {}
    orig_check = planner.replan_check

    def check_wrap(drone):
        n = len(planner.trajectory)
        pos = [np.array(q, dtype=np.float64) for q in planner.trajectory.positions]
        out = orig_check(drone)
        swep = np.array(out[1])
        # m: replan_check returns inside the loop at the first tracker hit, behind that waypoint's write
        m = n
        for i, q in enumerate(pos):
            if any(t.active and np.linalg.norm(t.estimate_pos(i * p.dt) - q) <= p.drone_radius + t.radius for t in drone.trackers):
                m = i + 1
                break
        seen.update(n=n, m=m, map=swep.astype(np.uint8))
        assert np.array_equal(seen['map'], swep), 'the returned map is not uint8-valued'
        return out
    planner.replan_check = check_wrap
    rec = {k: [] for k in ('action', 'n', 'm', 'map', 'crop')}
    done = False
    while not done:
        a = pol.plan(pol, env.info)
        a = 0.0 if a is None else float(a)
        _, _, done, _ = env.step(a)
        swep = seen['map']
        # envs/training_v3.py:206-209
        drone_idx = (int(env.drone.x // p.map_scale), int(env.drone.y // p.map_scale))
        edge_len = 2 * (p.drone_view_depth // p.map_scale)
        local = np.pad(swep, ((edge_len, edge_len), (edge_len, edge_len)), 'constant', constant_values=0)
        local = local[drone_idx[0]: drone_idx[0] + 2 * edge_len + 1, drone_idx[1]: drone_idx[1] + 2 * edge_len + 1]
        rec['action'].append(a)
        rec['n'].append(seen['n'])
        rec['m'].append(seen['m'])
        rec['map'].append(swep)
        rec['crop'].append(local.astype(np.uint8))
    dt = dict(action=np.float64, n=np.int32, m=np.int32, map=np.uint8, crop=np.uint8)
    out = {k: np.array(v, dtype=dt[k]) for k, v in rec.items()}
    out['cfg'] = np.array(json.dumps(kw))
    return out


def coverage(eps):
    """(truncated maps, empty-trajectory steps, longest trajectory, steps whose crop lost marked cells) over the episodes"""
    trunc = sum(int((d['m'] < d['n']).sum()) for d in eps)
    empty = sum(int((d['n'] == 0).sum()) for d in eps)
    longest = max(int(d['n'].max()) for d in eps)
    lost = sum(int((d['crop'].reshape(len(d['n']), -1).astype(np.int64).sum(1) != d['map'].reshape(len(d['n']), -1).astype(np.int64).sum(1)).sum())
               for d in eps)
    return trunc, empty, longest, lost


def main():
    warnings.simplefilter('ignore')
    out = {'episodes': np.array(len(EPISODES)), 'numpy_version': np.array(np.__version__)}
    eps = []
    for i, kw in enumerate(EPISODES):
        d = record(kw)
        eps.append(d)
        for k, v in d.items():
            out[f'e{i}_{k}'] = v
        print('map_id', kw['map_id'], 'steps', len(d['n']), 'truncated', int((d['m'] < d['n']).sum()), 'empty', int((d['n'] == 0).sum()),
              'longest', int(d['n'].max()), 'crop loses cells on', coverage([d])[3])
    trunc, empty, longest, lost = coverage(eps)
    assert trunc >= 5 and empty >= 5 and longest > 128 and lost >= 1, (trunc, empty, longest, lost)
    path = os.path.join(HERE, 'swept_episodes.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
