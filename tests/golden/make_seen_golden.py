#!/usr/bin/env python3
"""Recorder of tests/golden/seen_episodes.npz: yaw_planner.Oxford's `last_time_observed_map` (yaw_planner.py:49, :92-97) after every
plan() call of four whole episodes of the reference's gym-2d-perception-v2 env (envs/drone_v2.py) under --planner Primitive, the policy
called before every step as experiment.py:69 does, through make_golden.py's stubs.  Two episodes are flown with the policy's own
action and two with seeded random ones (the map is the policy's either way: it depends on the poses alone); one has a 120 degree view,
one starts in the interior of the map, where the crop of a learner's observation lies wholly inside it.

Per episode (prefix e<i>_): cfg (the parameters, JSON; `seed`: the random actions' seed, absent where the policy's action flew) and per
step
  action   the action the step was taken with
  pose     the drone's x, y and yaw as that plan() call found them
  map      Oxford.last_time_observed_map [W, H] float64 right after the plan() call in front of the step: entry t is the map of an env
           that has taken t steps
Episodes are shortened with max_flight_time, not thinned: every step is stored.  savez_compressed.  What is stored is data; runs only
where the reference is present.

Usage:  python tests/golden/make_seen_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

BASE = dict(gaze_method='Oxford', drone_max_speed=40, agent_max_speed=40, agent_radius=10)
EPISODES = [
    dict(BASE, map_id=0, agent_number=30, max_flight_time=10),
    dict(BASE, map_id=3, agent_number=30, max_flight_time=11, seed=17),
    dict(BASE, map_id=5, agent_number=10, max_flight_time=8, drone_view_range=120),
    dict(BASE, map_id=7, agent_number=6, max_flight_time=12, seed=23, init_pos=[250, 250], target_list=[[60, 440]]),
]
LIMIT = 200 * 1000        # bytes of the fixture


def record(kw):
    kw = dict(kw)
    seed = kw.get('seed')
    ref_kw = {k: v for k, v in kw.items() if k not in ('seed', 'init_pos', 'target_list')}
    p = G.make_params(planner='Primitive', **ref_kw)
    if 'init_pos' in kw:
        p.init_position = list(kw['init_pos'])
    if 'target_list' in kw:
        p.target_list = [list(t) for t in kw['target_list']]
    env = G.Drone2DEnv2(p)
    pol = G.yaw_planner.Oxford
    pol.__init__(pol, p)
    rs = np.random.RandomState(seed) if seed is not None else None
    rec = {'action': [], 'map': [], 'pose': []}
    done = False
    while not done:
        a = pol.plan(pol, env.info)
        a = 0.0 if a is None else float(a)
        if rs is not None:
            a = float(rs.uniform(-1, 1))
        rec['map'].append(np.array(pol.last_time_observed_map, dtype=np.float64))
        rec['action'].append(a)
        rec['pose'].append([env.drone.x, env.drone.y, env.drone.yaw])
        _, _, done, _ = env.step(a)
    out = {k: np.array(v, dtype=np.float64) for k, v in rec.items()}
    out['cfg'] = np.array(json.dumps(kw))
    return out, p


def main():
    warnings.simplefilter('ignore')
    out = {'episodes': np.array(len(EPISODES)), 'numpy_version': np.array(np.__version__)}
    for i, kw in enumerate(EPISODES):
        d, p = record(kw)
        for k, v in d.items():
            out[f'e{i}_{k}'] = v
        print('map_id', kw['map_id'], 'steps', len(d['action']), 'bytes raw', d['map'].nbytes)
    path = os.path.join(HERE, 'seen_episodes.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < LIMIT, size
    # the coverage the fixture is for, from the file itself (tests/seen_cases.coverage re-asserts it)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import seen_cases as SC
    cov = SC.coverage()
    print('re-seen cells, in-map crops, never-seen cells in a crop:', cov)
    assert cov[0] >= 100 and cov[1] >= 20 and cov[2] >= 1, cov


if __name__ == '__main__':
    main()
