#!/usr/bin/env python3
"""Recorder of tests/golden/tracks_episodes.npz: the Kalman trackers after every step of four whole episodes of the reference's
gym-2d-perception-v2 env (envs/drone_v2.py) under seeded random gaze actions, and the window of the tracker-forecast map
(include/d2d_tracks.h) computed literally from the reference's own functions, through make_golden.py's stubs.

  (a) Primitive / CVM, 10 agents, the default 90 degree view: a tracker stays active after its forecast has left the window
  (b) Primitive / RVO, 15 agents                          (c) Jerk_Primitive / CVM with var_cam = 2, 15 agents
  (d) Primitive / CVM from a start 30 px off the map's corner, 12 agents
(b) to (d) with a 120 degree view, so that several agents are tracked at once.

Per episode (prefix e<i>_): cfg (the parameters, JSON; `seed`: the actions' seed) and per step, as the step left the env,
  action   the action the step was taken with
  pose     the drone's x, y and yaw
  active   [N] uint8, tracker.active
  mu       [N, 4] float64, tracker.mu_upds[-1]
  radius   [N] float64, tracker.radius
  win      [L, L] uint8: F for margin = 5 + var_cam and 31 samples, zero-padded and cut around the drone's cell as
           envs/training_v3.py:206-209 does it.  F[i, j] = 1 + the first k in 0 .. 30 with
           numpy.linalg.norm(map.get_real_pos(i, j) - tracker.estimate_pos(k * dt)) <= drone_radius + tracker.radius + margin for an
           active tracker, 0 where there is none: evaluated with exactly these calls on every cell within the threshold plus two cells
           of the forecast along both axes (no other cell can pass the test)
  win0     the same for margin = 0, every tenth step (steps 0, 10, ...)
With them the tie table of the recording host's np.argsort (drone2d_amd.jerk_plugin.tie_table) for the Jerk_Primitive episode.
savez_compressed.  What is stored is data; runs only where the reference is present.

Usage:  python tests/golden/make_tracks_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

BASE = dict(agent_radius=10, agent_max_speed=40, drone_max_speed=40, drone_view_range=120)
EPISODES = [
    dict(BASE, planner='Primitive', agent_number=10, drone_view_range=90, map_id=0, max_flight_time=10, seed=41),
    dict(BASE, planner='Primitive', motion_profile='RVO', agent_number=15, map_id=5, max_flight_time=8, seed=43),
    dict(BASE, planner='Jerk_Primitive', agent_number=15, map_id=5, max_flight_time=8, var_cam=2, seed=47),
    dict(BASE, planner='Primitive', agent_number=12, map_id=1, max_flight_time=8, seed=53, init_pos=[30, 30], target_list=[[440, 440]]),
]
SAMPLES = 31
LIMIT = 200 * 1000        # bytes of the fixture
NOT_PARAMS = ('seed', 'init_pos', 'target_list')


def forecast(env, p, margin):
    """F [W, H] of the env as it stands, from get_real_pos, estimate_pos and norm"""
    from numpy.linalg import norm
    gmap = env.drone.map
    W, H = gmap.grid_map.shape
    F = np.zeros((W, H), dtype=np.int64)
    for tr in env.drone.trackers:
        if not tr.active:
            continue
        thr = p.drone_radius + tr.radius + margin
        for k in range(SAMPLES):
            est = tr.estimate_pos(k * p.dt)
            if not np.all(np.isfinite(est)):
                continue
            reach = thr + 2 * p.map_scale
            i_lo, i_hi = int((est[0] - reach) // p.map_scale), int((est[0] + reach) // p.map_scale)
            j_lo, j_hi = int((est[1] - reach) // p.map_scale), int((est[1] + reach) // p.map_scale)
            for i in range(max(i_lo, 0), min(i_hi, W - 1) + 1):
                for j in range(max(j_lo, 0), min(j_hi, H - 1) + 1):
                    if norm(gmap.get_real_pos(i, j) - est) <= thr and (F[i, j] == 0 or F[i, j] > k + 1):
                        F[i, j] = k + 1
    return F


def window(env, p, F):
    """envs/training_v3.py:206-209"""
    drone_idx = (int(env.drone.x // p.map_scale), int(env.drone.y // p.map_scale))
    edge_len = 2 * (p.drone_view_depth // p.map_scale)
    local = np.pad(F, ((edge_len, edge_len), (edge_len, edge_len)), 'constant', constant_values=0)
    local = local[drone_idx[0]: drone_idx[0] + 2 * edge_len + 1, drone_idx[1]: drone_idx[1] + 2 * edge_len + 1]
    assert local.max() <= 255
    return local.astype(np.uint8)


def record(kw):
    kw = dict(kw)
    p = G.make_params(**{k: v for k, v in kw.items() if k not in NOT_PARAMS})
    if 'init_pos' in kw:
        p.init_position = list(kw['init_pos'])
    if 'target_list' in kw:
        p.target_list = [list(t) for t in kw['target_list']]
    env = G.Drone2DEnv2(p)
    rs = np.random.RandomState(kw['seed'])
    rec = {k: [] for k in ('action', 'pose', 'active', 'mu', 'radius', 'win', 'win0')}
    done, t = False, 0
    while not done:
        a = float(rs.uniform(-1, 1))
        _, _, done, _ = env.step(a)
        N = len(env.agents)                  # (the drone allocates more trackers than there are agents: the rest never activate)
        assert not any(tr.active for tr in env.drone.trackers[N:])
        trs = env.drone.trackers[:N]
        rec['action'].append(a)
        rec['pose'].append([env.drone.x, env.drone.y, float(np.asarray(env.drone.yaw).ravel()[0])])
        rec['active'].append([bool(tr.active) for tr in trs])
        rec['mu'].append([np.asarray(tr.mu_upds[-1], dtype=np.float64).reshape(4) for tr in trs])
        rec['radius'].append([float(tr.radius) for tr in trs])
        rec['win'].append(window(env, p, forecast(env, p, 5 + p.var_cam)))
        if t % 10 == 0:
            rec['win0'].append(window(env, p, forecast(env, p, 0)))
        t += 1
    dt = dict(active=np.uint8, win=np.uint8, win0=np.uint8)
    out = {k: np.array(v, dtype=dt.get(k, np.float64)) for k, v in rec.items()}
    out['cfg'] = np.array(json.dumps(kw))
    return out


def main():
    warnings.simplefilter('ignore')
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from drone2d_amd import jerk_plugin as JP
    perm, eq = JP.tie_table()
    out = {'episodes': np.array(len(EPISODES)), 'numpy_version': np.array(np.__version__), 'tie_perm': perm, 'tie_eq': eq}
    for i, kw in enumerate(EPISODES):
        d = record(kw)
        for k, v in d.items():
            out[f'e{i}_{k}'] = v
        print('map_id', kw['map_id'], 'steps', len(d['action']), 'nonzero windows', int((d['win'].reshape(len(d['win']), -1).any(1)).sum()),
              'active at most', int(d['active'].sum(1).max()))
    path = os.path.join(HERE, 'tracks_episodes.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < LIMIT, size
    # the coverage the fixture is for, from the file itself (tests/tracks_cases.coverage re-asserts it)
    import tracks_cases as TC
    cov = TC.coverage()
    print(cov)
    TC.assert_coverage(cov)


if __name__ == '__main__':
    main()
