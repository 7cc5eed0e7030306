#!/usr/bin/env python3
"""Golden Owl episodes: runs the REAL reference (imported through make_golden.py's stubs) under yaw_planner.Owl with the
Primitive planner and stores arrays only -- per step the policy's action and Owl.U_list after the plan() call, per episode the
CSV row -- as owl_episodes.npz next to this script.  Six episodes the two Owl cases of host_gaze_rows.npz do not cover: a 120
degree view 100 px deep, pillars, a static map, two targets, a fast drone, a non-square map.

Runs only where the reference is present (like make_golden.py).

Usage:  python tests/golden/make_golden_owl.py
"""
import json
import warnings

import numpy as np

import make_golden as MG

BASE = dict(gaze_method='Owl', planner='Primitive', agent_number=10, agent_max_speed=20, agent_radius=15, drone_max_speed=40)
CASES = [
    ('fov120_depth100', dict(BASE, drone_view_range=120, drone_view_depth=100, agent_number=20, agent_max_speed=40, map_id=11)),
    ('pillars', dict(BASE, pillar_number=4, agent_radius=10, map_id=12)),
    ('static_map', dict(BASE, static_map='maps/obstacle_map.npy', agent_radius=10, map_id=13)),
    ('two_targets', dict(BASE, target_list=[[420, 100], [100, 420]], agent_number=20, agent_radius=10, map_id=14)),
    ('fast_drone', dict(BASE, drone_max_speed=60, agent_number=30, agent_max_speed=40, agent_radius=10, map_id=15)),
    ('map700x400', dict(BASE, map_size=[700, 400], init_pos=[60, 60], target_list=[[640, 340]], agent_number=20,
                        agent_radius=10, map_id=16)),
]


def owl_episode(params):
    """One episode driven like Experiment.run: (actions [T], U_list after every plan() [T][36], the CSV row's values)"""
    env = MG.Drone2DEnv2(params)
    pol = MG.yaw_planner.Owl
    pol.__init__(pol, params)
    acts, scores, done, info = [], [], False, None
    while not done:
        a = pol.plan(pol, env.info)
        acts.append(float(a))
        scores.append(np.array(pol.U_list, dtype=np.float64))
        _, _, done, info = env.step(a)
    buf = info['tracker_buffer']
    n = len(buf)
    gm = info['drone'].map.grid_map
    row = [info['flight_time'], float(gm.size - np.count_nonzero(gm == 0)), n,
           float(sum(len(t.ts) * 0.1 for t in buf) / n) if n else float('nan'),
           int(info['state_machine'] == 1), int(info['collision_flag'] == 1), int(info['collision_flag'] == 2),
           info['freezing_flag'], info['dead_lock_flag'], info['state_machine']]
    return np.array(acts), np.array(scores), np.array(row, dtype=np.float64)


def main():
    warnings.simplefilter('ignore')                      # Owl divides by the speed of a drone at rest
    d = {'n': np.array(len(CASES)), 'names': np.array([n for n, _ in CASES])}
    for i, (name, kw) in enumerate(CASES):
        acts, scores, row = owl_episode(MG.make_params(**kw))
        d[f'r{i}_cfg'], d[f'r{i}_actions'], d[f'r{i}_scores'], d[f'r{i}_row'] = np.array(json.dumps(kw)), acts, scores, row
        print(name, len(acts), 'steps', len(set(acts.tolist())), 'distinct actions', row)
    MG.save('owl_episodes', d)


if __name__ == '__main__':
    main()
