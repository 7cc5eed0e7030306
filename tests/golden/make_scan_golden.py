#!/usr/bin/env python3
"""Recorder of tests/golden/scan_episodes.npz: `env.drone.rays` (utils.py:712, :746) after every step of four episodes of the
reference's gym-2d-perception-v2 env (envs/drone_v2.py), through make_golden.py's stubs.

  (a) NoMove, 40 agents of radius 15 at speed 20, map_id 7, 40 steps, stepped on past `done`; the drone is put somewhere before every
      step, an 8-pose cycle: a corner with yaw 45 t, next to the right wall, an agent's rounded centre, the middle with yaw 4 t, on the
      map's edge (x = 0: no ray takes a sample), 30 px left of an agent looking at it, next to the bottom wall looking at it, a
      drifting point with yaw 45 t + 22.5
  (b) Primitive / CVM, 10 agents of radius 10 at speed 40, drone_max_speed 40, 60 steps of seeded random actions
  (c) Primitive / RVO, 10 agents, map_id 4, to the episode's end
  (d) NoMove on a map of 1000 x 800 px with depth 120 and a 120 degree view, 40 agents, 20 steps, the drone put somewhere before every
      step: 100 rays and two hit words

Per episode (prefix e<i>_): cfg (the parameters, JSON; `seed`: the random actions' seed) and per step
  action   the action the step was taken with
  tele     x, y, yaw the drone was given in front of the step (NaN: it was left where it was)
  pose     the drone's x, y and yaw as the step found them
  coords   [R, 2] float64, 'coords' of every ray
  wall     [R] uint8, 'wall' of every ray: the raw map_gt value at a range stop
  hit      [R, words] uint32, 'hit_list' packed: bit k % 32 of word k / 32
Every step is stored.  savez_compressed.  What is stored is data; runs only where the reference is present.

Usage:  python tests/golden/make_scan_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

EPISODES = [
    dict(planner='NoMove', agent_number=40, agent_radius=15, agent_max_speed=20, map_id=7, steps=40, teleport='cycle'),
    dict(planner='Primitive', agent_number=10, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=0, steps=60, seed=31),
    dict(planner='Primitive', motion_profile='RVO', agent_number=10, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=4, seed=37),
    dict(planner='NoMove', agent_number=40, agent_radius=15, agent_max_speed=20, map_id=11, steps=20, teleport='wide', map_size=[1000, 800],
         drone_view_depth=120, drone_view_range=120, init_pos=[100, 100], target_list=[[900, 700]]),
]
LIMIT = 200 * 1000        # bytes of the fixture
NOT_PARAMS = ('seed', 'steps', 'teleport')


def _agent(env, k, margin):
    """(rounded x, rounded y) of the first agent from index k on that lies `margin` px inside the map on every side"""
    n = len(env.agents)
    w, h = env.params.map_size
    for d in range(n):
        x, y = (int(round(float(v))) for v in env.agents[(k + d) % n].position)
        if margin < x < w - margin and margin < y < h - margin:
            return x, y
    raise AssertionError('no agent inside the margin')


def _closest_pair_member(env):
    pos = np.array([a.position for a in env.agents], dtype=np.float64)
    d = ((pos[:, None] - pos[None]) ** 2).sum(-1) + np.eye(len(pos)) * 1e12
    return int(np.unravel_index(np.argmin(d), d.shape)[0])


def cycle_pose(env, t):
    k = t % 8
    if k == 0:
        return 15, 15, (45 * t) % 360
    if k == 1:
        return 485, 250, (13 * t) % 360
    if k == 2:
        x, y = _agent(env, _closest_pair_member(env) if (t // 8) % 2 == 0 else t // 8, 2)
        return x, y, (30 * t) % 360
    if k == 3:
        return 250, 250, (4 * t) % 360
    if k == 4:
        return 0, 100, 90
    if k == 5:
        x, y = _agent(env, t // 8, 40)
        return x - 30, y, 0
    if k == 6:
        return 250, 490, 270
    return 100 + 7 * t, 400 - 5 * t, (45 * t + 22.5) % 360


def wide_pose(env, t):
    rs = np.random.RandomState(100 + t)
    if t % 4 == 0:
        x, y = _agent(env, 20 + t, 40)
        return x - 30, y, 0
    if t % 4 == 1:
        x, y = _agent(env, 20 + t, 2)
        return x, y, int(rs.randint(0, 360))
    if t % 4 == 2:
        return int(rs.randint(1, 1000)), int(rs.randint(1, 800)), float(rs.uniform(0, 360))
    return [(5, 5, 315), (995, 795, 135), (500, 795, 270), (995, 400, 0), (500, 400, 60)][t // 4]


def record(kw):
    kw = dict(kw)
    seed, steps, tele = kw.get('seed'), kw.get('steps'), kw.get('teleport')
    p = G.make_params(**{k: v for k, v in kw.items() if k not in NOT_PARAMS})
    env = G.Drone2DEnv2(p)
    rs = np.random.RandomState(seed) if seed is not None else None
    rec = {k: [] for k in ('action', 'tele', 'pose', 'coords', 'wall', 'hit')}
    N = len(env.agents)
    words = max(1, (N + 31) // 32)
    done, t = False, 0
    while (t < steps) if steps is not None else (not done):
        a = float(rs.uniform(-1, 1)) if rs is not None else 0.0
        if tele is not None:
            x, y, yaw = (cycle_pose if tele == 'cycle' else wide_pose)(env, t)
            env.drone.x, env.drone.y, env.drone.yaw = x, y, yaw
            rec['tele'].append([x, y, yaw])
        else:
            rec['tele'].append([np.nan] * 3)
        rec['pose'].append([env.drone.x, env.drone.y, float(np.asarray(env.drone.yaw).ravel()[0])])
        _, _, done, _ = env.step(a)
        rays = env.drone.rays
        rec['action'].append(a)
        rec['coords'].append([[float(r['coords'][0]), float(r['coords'][1])] for r in rays])
        rec['wall'].append([int(r['wall']) for r in rays])
        hit = np.zeros((len(rays), words), dtype=np.uint32)
        for i, r in enumerate(rays):
            for k in np.nonzero(r['hit_list'].numpy())[0]:
                hit[i, k >> 5] |= np.uint32(1 << (int(k) & 31))
        rec['hit'].append(hit)
        t += 1
    if steps is not None and tele is None:
        assert not done or t == steps, ('the episode ended before its last recorded step', t)
    out = {k: np.array(rec[k], dtype=np.float64) for k in ('action', 'tele', 'pose', 'coords')}
    out['wall'] = np.array(rec['wall'], dtype=np.uint8)
    out['hit'] = np.array(rec['hit'], dtype=np.uint32)
    out['cfg'] = np.array(json.dumps(kw))
    return out


def main():
    warnings.simplefilter('ignore')
    out = {'episodes': np.array(len(EPISODES)), 'numpy_version': np.array(np.__version__)}
    for i, kw in enumerate(EPISODES):
        d = record(kw)
        for k, v in d.items():
            out[f'e{i}_{k}'] = v
        print('map_id', kw['map_id'], 'steps', len(d['action']), 'rays', d['wall'].shape[1], 'hit words', d['hit'].shape[2])
    path = os.path.join(HERE, 'scan_episodes.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < LIMIT, size
    # the coverage the fixture is for, from the file itself (tests/scan_cases.coverage re-asserts it)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import scan_cases as SC
    cov = SC.coverage()
    print(cov)
    SC.assert_coverage(cov)


if __name__ == '__main__':
    main()
