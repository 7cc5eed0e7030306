#!/usr/bin/env python3
"""Recorder of tests/golden/rvo_traces.npz: the reference env under --motion_profile RVO, stepped through make_golden.py's stubs.

Per world (prefix w<i>_): the initial agents (position, velocity, preferred velocity, radius), the pillars, and per step the
agents' position, velocity and preferred velocity and `done`; for the worlds listed in FULL also every step output that
make_golden.run_trace records (prefix w<i>_full_); the seconds per step the reference took on the recording machine.  One
Primitive + LookAhead episode is stored as its CSV row and per-step actions.  What is stored is data; runs only where the
reference is present.

Usage:  python tests/golden/make_rvo_golden.py
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

T_MAX = 40
WORLDS = [
    ('readme', dict(agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1), 40),
    ('pillars300', dict(agent_number=12, agent_radius=12, agent_max_speed=30, pillar_number=6, map_size=[300, 300], map_id=5,
                        init_pos=[40, 40], target_list=[[260, 260]]), 40),
    ('n30', dict(agent_number=30, agent_radius=15, agent_max_speed=20, map_id=2), 40),
    ('obstacle_map', dict(agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1, static_map='maps/obstacle_map.npy'), 12),
    ('one_agent', dict(agent_number=1, agent_radius=15, agent_max_speed=20, map_id=3), 40),
    ('one_agent_pillars', dict(agent_number=1, agent_radius=15, agent_max_speed=20, map_id=3, pillar_number=3), 40),
]
FULL = ('readme', 'pillars300')
EPISODE = dict(gaze_method='LookAhead', planner='Primitive', agent_number=20, agent_radius=8, agent_max_speed=40, map_id=7,
               drone_max_speed=40)


def agents_of(env):
    ag = env.agents
    N = len(ag)
    return (np.array([a.position for a in ag], dtype=np.float64).reshape(N, 2),
            np.array([a.velocity for a in ag], dtype=np.float64).reshape(N, 2),
            np.array([a.pref_velocity for a in ag], dtype=np.float64).reshape(N, 2))


def record(name, kw, T):
    p = G.make_params(planner='NoMove', motion_profile='RVO', **kw)
    rng = np.random.RandomState(len(name))
    actions = rng.uniform(-1, 1, T)
    seen = {'vel': []}

    def watch(env, t):
        seen['env'] = env
        if t > 0:
            seen['vel'].append(agents_of(env)[1])
    t0 = time.perf_counter()
    tr = G.run_trace(p, T, actions=actions, stop_on_done=False, mutate=watch)
    seconds = (time.perf_counter() - t0) / T
    seen['vel'].append(agents_of(seen['env'])[1])
    d = {k: tr[k] for k in ('agent_pos', 'agent_vel', 'agent_pref', 'agent_radius', 'obstacles')}
    d.update(t_agent_pos=tr['t_agent_pos'], t_agent_pref=tr['t_agent_pref'], t_agent_vel=np.array(seen['vel']),
             t_done=tr['t_done'], params_json=tr['params_json'], cfg=np.array(json.dumps(kw)), ref_seconds_per_step=np.array(seconds))
    if name in FULL:
        for k, v in tr.items():
            if k not in d:
                d['full_' + k] = v
    return d


def episode():
    acts = []
    t0 = time.perf_counter()
    row = G.experiment_row(G.make_params(motion_profile='RVO', **EPISODE), 'LookAhead', acts)
    return dict(ep_cfg=np.array(json.dumps(EPISODE)), ep_row=np.array(row, dtype=np.float64), ep_actions=np.array(acts, dtype=np.float64),
                ep_ref_seconds_per_step=np.array((time.perf_counter() - t0) / max(len(acts), 1)))


def main():
    out = {'names': np.array([w[0] for w in WORLDS])}
    for i, (name, kw, T) in enumerate(WORLDS):
        assert T <= T_MAX
        for k, v in record(name, kw, T).items():
            out[f'w{i}_{k}'] = v
        print(name, 'N', len(out[f'w{i}_agent_pos']), 'P', len(out[f'w{i}_obstacles']), 'T', len(out[f'w{i}_t_done']),
              f"{float(out[f'w{i}_ref_seconds_per_step']):.4f} s/step")
    out.update(episode())
    print('episode', len(out['ep_actions']), 'steps', out['ep_row'])
    G.save('rvo_traces', out)


if __name__ == '__main__':
    main()
