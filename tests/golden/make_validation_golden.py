#!/usr/bin/env python3
"""Recorder of tests/golden/validation_episodes.npz: a dozen episodes of the reference's validation study, played the way its scripts
play them, through make_golden.py's stubs (the reference is imported at run time; what is stored is data).

  'speed' form   script/validation_speed.py: agent_radius 5 / 15 at the default agent speed, (Primitive, Oxford); per episode
                 gym.make -> env.reset() -> every agent's pref_velocity redrawn from `random` -> the policy loop.  The row's
                 'Agent speed' is the script's -1.
  'size' form    script/validation_size.py: agent_radius = -1 at agent_max_speed 20 / 60, (Jerk_Primitive, NoControl) through
                 Experiment.run (view range 360, experiment.py:28-29), which redraws nothing.  For these worlds the redraw is recorded
                 too (x_pairs, x_pref: env.reset() and the three lines, no episode), so that a world with random radii is covered.

Per episode (prefix e<i>_): cfg (json: form, the Params fields, start, target, redraw), N, py_pos (position of the `random` stream
after env.reset(): the redraw crosses a key regeneration where py_pos + 4 N > 624), pairs [N, 2] (the raw random() of the redraw),
pref [N, 2] (the redrawn pref_velocity), row (flight time, grid discovered, agents tracked, mean tracked time, success, static
collision, dynamic collision, freezing, dead lock, state machine) and, where it was played, row_plain: the row of the same episode
without the redraw.  With the episodes: the tie table of the recording host's np.argsort and its numpy version, as in jerk_traces.npz.

The generator asserts what the fixture is for: a world with the static map's cell agents, a redraw that crosses a regeneration, two
outcomes, and a row that differs from the row without the redraw.

Usage:  python tests/golden/make_validation_golden.py
"""
import json
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

gym = sys.modules['gym']
gym.make = lambda name, params: G.Drone2DEnv2(params)          # the registered id of both scripts is this class

T_MAX = 12                                                      # max_flight_time of every episode: 121 steps at the most
SPEED = dict(form='speed', agent_number=10, agent_max_speed=40, drone_max_speed=40, static_map='maps/empty_map.npy', redraw=True)
SIZE = dict(form='size', agent_number=10, agent_radius=-1, drone_max_speed=40, static_map='maps/empty_map.npy', redraw=False)
EPISODES = [
    dict(SPEED, agent_radius=5, map_id=0, start=(40, 40), target=(250, 250), plain=True),
    dict(SPEED, agent_radius=5, map_id=1, start=(460, 460), target=(40, 250), plain=True),
    dict(SPEED, agent_radius=5, map_id=2, start=(250, 40), target=(250, 460), drone_max_speed=60),
    dict(SPEED, agent_radius=15, map_id=0, start=(40, 40), target=(460, 460), plain=True),
    dict(SPEED, agent_radius=15, map_id=3, start=(40, 460), target=(250, 250), plain=True),
    dict(SPEED, agent_radius=15, map_id=4, start=(250, 250), target=(40, 40), drone_max_speed=20),
    dict(SPEED, agent_radius=15, map_id=1, start=(40, 250), target=(460, 250), static_map='maps/obstacle_map.npy'),
    dict(SPEED, agent_radius=5, map_id=None, agent_number=90, start=(40, 40), target=(250, 40)),     # map_id: the crossing search
    #   (90 agents take some 95 attempts of six words: the stream then stands near the end of its first key)
    dict(SIZE, agent_max_speed=20, map_id=0, start=(40, 40), target=(250, 250)),
    dict(SIZE, agent_max_speed=60, map_id=1, start=(460, 250), target=(40, 40)),
    dict(SIZE, agent_max_speed=60, map_id=2, agent_number=30, start=(250, 460), target=(250, 40)),
]
POLICY = {'speed': ('Primitive', 'Oxford'), 'size': ('Jerk_Primitive', 'NoControl')}


def study_params(c):
    """the Params of the scripts' outer loop (validation_speed.py:49-55, validation_size.py:30-37)"""
    p = G.Params(debug=True, map_id=c['map_id'], gaze_method='NoControl', planner='NoMove', agent_number=c['agent_number'],
                 agent_radius=c['agent_radius'], agent_max_speed=c['agent_max_speed'], static_map=c['static_map'], max_flight_time=T_MAX)
    p.render = False
    return p


def redraw(env):
    """validation_speed.py:135-138, keeping the raw draws"""
    pairs = []
    for agent in env.agents:
        r0 = random.random()
        vel = r0 * 40 + 20
        r1 = random.random()
        angle = r1 * 2 * np.pi
        agent.pref_velocity = np.array([vel * np.cos(angle), vel * np.sin(angle)])
        pairs.append((r0, r1))
    return np.array(pairs, dtype=np.float64).reshape(-1, 2)


def play(c, with_redraw):
    planner, gaze = POLICY[c['form']]
    params = study_params(c)
    gym.make('gym-2d-perception-v2', params=params)
    params.gaze_method, params.planner, params.drone_max_speed = gaze, planner, c['drone_max_speed']
    params.init_position, params.target_list, params.record = c['start'], [c['target']], True
    if gaze == 'NoControl':
        params.drone_view_range = 360                              # experiment.py:28-29
    policy = getattr(G.yaw_planner, gaze)
    policy.__init__(policy, params)
    env = gym.make('gym-2d-perception-v2', params=params)
    env.reset()
    out = dict(N=np.array(len(env.agents)), py_pos=np.array(random.getstate()[1][-1]))
    if with_redraw:
        out['pairs'] = redraw(env)
        out['pref'] = np.array([a.pref_velocity for a in env.agents], dtype=np.float64).reshape(-1, 2)
    done, info = False, None
    while not done:
        a = policy.plan(policy, env.info)
        _, _, done, info = env.step(a)
    buf = info['tracker_buffer']
    n = len(buf)
    gm = info['drone'].map.grid_map
    out['row'] = np.array([info['flight_time'], float(gm.shape[0] * gm.shape[1] - np.sum(np.where(gm == 0, 1, 0))), n,
                           float(np.array([len(t.ts) * 0.1 for t in buf]).sum() / n) if n else float('nan'),
                           1 if info['state_machine'] == 1 else 0, 1 if info['collision_flag'] == 1 else 0,
                           1 if info['collision_flag'] == 2 else 0, info['freezing_flag'], info['dead_lock_flag'],
                           info['state_machine']], dtype=np.float64)
    return out


def redrawn_world(c):
    """env.reset() and the redraw alone, for a world whose episode the script plays without it"""
    params = study_params(c)
    params.init_position, params.target_list = c['start'], [c['target']]
    env = gym.make('gym-2d-perception-v2', params=params)
    env.reset()
    pos = random.getstate()[1][-1]
    pairs = redraw(env)
    return pos, pairs, np.array([a.pref_velocity for a in env.agents], dtype=np.float64).reshape(-1, 2)


def crossing_map_id(c):
    """the first map id whose `random` stream stands, after env.reset(), where the 4 N words of the redraw run past the key"""
    for m in range(200):
        q = dict(c, map_id=m)
        params = study_params(q)
        params.init_position, params.target_list = q['start'], [q['target']]
        env = gym.make('gym-2d-perception-v2', params=params)
        env.reset()
        if random.getstate()[1][-1] + 4 * len(env.agents) > 624:
            return m
    raise SystemExit('no crossing world among 200 map ids')


def main():
    warnings.simplefilter('ignore')
    from drone2d_amd import jerk_plugin as JP
    perm, eq = JP.tie_table()
    out = {'n': np.array(len(EPISODES)), 'tie_perm': perm, 'tie_eq': eq, 'numpy_version': np.array(np.__version__)}
    differs, crosses, cells, outcomes = 0, 0, 0, set()
    for i, c in enumerate(EPISODES):
        c = dict(c)
        plain = c.pop('plain', False)
        if c['map_id'] is None:
            c['map_id'] = crossing_map_id(c)
        d = play(c, c['redraw'])
        if plain:
            d['row_plain'] = play(c, False)['row']
            same = np.array_equal(d['row'], d['row_plain'], equal_nan=True)
            differs += not same
        if not c['redraw']:
            pos, d['x_pairs'], d['x_pref'] = redrawn_world(c)
            assert pos == int(d['py_pos'])
        N, pos = int(d['N']), int(d['py_pos'])
        crosses += bool(c['redraw'] and pos + 4 * N > 624)
        cells += bool(c['redraw'] and N > c['agent_number'])
        outcomes.add(tuple(d['row'][4:9].astype(int)))
        for k, v in d.items():
            out[f'e{i}_{k}'] = v
        out[f'e{i}_cfg'] = np.array(json.dumps(dict(c, max_flight_time=T_MAX)))
        print(i, c['form'], 'map', c['map_id'], 'N', N, 'pos', pos, 'row', d['row'].tolist(),
              'plain', d['row_plain'].tolist() if plain else None, flush=True)
    assert differs >= 1, 'no row differs from the row of the same world without the redraw'
    assert crosses >= 1, 'no redraw crosses a key regeneration'
    assert cells >= 1, 'no redrawn world holds cell agents of a static map'
    assert len(outcomes) >= 2, outcomes
    G.save('validation_episodes', out)


if __name__ == '__main__':
    main()
