#!/usr/bin/env python3
"""Recorder of tests/golden/jerk_gaze_episodes.npz: whole episodes of the reference under --planner Jerk_Primitive, driven as
experiment.py:65-70 drives them -- policy.__init__(policy, params); while not done: a = policy.plan(policy, env.info); env.step(a) --
through make_golden.py's stubs.

Per world (prefix w<i>_): the parameters, N, the CSV row of experiment.py:73-103 (`row`: flight time, grid discovered, agents tracked,
mean tracked time, success, static collision, dynamic collision, freezing, dead lock, state machine) and per step
  what the policy saw   g_drone (x, y, yaw, vx, vy), g_target, g_active, g_mu (every tracker's latest mean)
  what it answered      action; for Owl: owl_U (U_list after the call), owl_left (len(Owl.u)), owl_rate (the yaw rate it holds)
  what plan() gave      plan_ok, choice (theta / 5 of the primitive taken, -1 when it failed)
  the env afterwards    drone (x, y, yaw), vel (velocity, acceleration), sm, fail, flags, done
With the episodes: the tie table of the recording host's np.argsort (drone2d_amd.jerk_plugin.tie_table) and its numpy version, as in
jerk_traces.npz.  What is stored is data; runs only where the reference is present.

The dead-lock world: map ids of a crowded, slow world are searched for an episode that ends with dead_lock_flag; main() prints what
the search found.

Usage:  python tests/golden/make_jerk_gaze_golden.py [--no-search]
"""
import json
import math
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

BASE = dict(agent_number=10, agent_radius=15, agent_max_speed=20, max_flight_time=12)
WORLDS = [
    ('lookahead40', dict(BASE, gaze_method='LookAhead', drone_max_speed=40, map_id=0)),
    ('lookahead20', dict(BASE, gaze_method='LookAhead', drone_max_speed=20, map_id=1, max_flight_time=25)),
    ('owl40', dict(BASE, gaze_method='Owl', drone_max_speed=40, map_id=2)),
    ('owl20', dict(BASE, gaze_method='Owl', drone_max_speed=20, map_id=3, max_flight_time=25)),
    ('owl_var_cam2', dict(BASE, gaze_method='Owl', drone_max_speed=40, map_id=4, var_cam=2)),
    ('owl_obstacle_map', dict(BASE, gaze_method='Owl', drone_max_speed=40, map_id=5, static_map='maps/obstacle_map.npy', agent_number=4,
                              agent_radius=10)),
    ('owl_rvo', dict(BASE, gaze_method='Owl', drone_max_speed=40, map_id=6, motion_profile='RVO')),
    ('lookgoal', dict(BASE, gaze_method='LookGoal', drone_max_speed=40, map_id=7)),
    ('oxford', dict(BASE, gaze_method='Oxford', drone_max_speed=40, map_id=8)),
    ('nocontrol', dict(BASE, gaze_method='NoControl', drone_max_speed=40, map_id=9)),
    ('rotating', dict(BASE, gaze_method='Rotating', drone_max_speed=40, map_id=10)),
    ('freezing', dict(BASE, gaze_method='Owl', drone_max_speed=20, map_id=11, max_flight_time=8, target_list=[[450, 450]])),
]
DEADLOCK = dict(gaze_method='Owl', drone_max_speed=20, agent_number=30, agent_radius=20, agent_max_speed=5, max_flight_time=15)
DEADLOCK_IDS = range(0, 60)


def record(kw):
    from drone2d_amd import jerk_plugin as JP
    p = G.make_params(planner='Jerk_Primitive', **kw)
    if p.gaze_method == 'NoControl':
        p.drone_view_range = 360                                   # experiment.py:28-29
    env = G.Drone2DEnv2(p)
    pol = getattr(G.yaw_planner, p.gaze_method)
    pol.__init__(pol, p)
    N = len(env.agents)
    planner = env.planner
    seen = {}
    orig_plan, orig_prim = planner.plan, planner.generate_primitive

    def prim_wrap(p0, v0, a0, theta_h, v_max, delt_t):
        seen['theta'] = float(theta_h)
        return orig_prim(p0, v0, a0, theta_h, v_max, delt_t)

    def plan_wrap(drone, dt):
        seen['phi'] = math.degrees(math.atan2(planner.target[1] - drone.y, planner.target[0] - drone.x))
        seen['ok'] = bool(orig_plan(drone, dt))
        return seen['ok']
    planner.plan, planner.generate_primitive = plan_wrap, prim_wrap
    keys = ('g_drone', 'g_target', 'g_active', 'g_mu', 'action', 'owl_U', 'owl_left', 'owl_rate', 'plan_ok', 'choice', 'drone', 'vel',
            'sm', 'fail', 'flags', 'done', 'unknown')
    rec = {k: [] for k in keys}
    perm, eq = tie_table()
    done, info, held = False, None, 0.0
    while not done:
        obs = env.info
        d, trk = obs['drone'], obs['drone'].trackers[:N]
        rec['g_drone'].append([d.x, d.y, float(np.asarray(d.yaw).ravel()[0])] + [float(v) for v in np.asarray(d.velocity).ravel()])
        rec['g_target'].append([float(obs['target'][0]), float(obs['target'][1])])
        rec['g_active'].append([t.active is True for t in trk])
        rec['g_mu'].append(np.array([t.mu_upds[-1][:, 0] for t in trk], dtype=np.float64).reshape(N, 4))
        a = pol.plan(pol, obs)
        rec['action'].append(float(a))
        if p.gaze_method == 'Owl':
            if len(pol.u):
                held = float(pol.u[-1])
            rec['owl_U'].append(np.array(pol.U_list, dtype=np.float64))
            rec['owl_left'].append(len(pol.u))
            rec['owl_rate'].append(held)
        _, _, done, info = env.step(a)
        rec['plan_ok'].append(seen['ok'])
        rec['choice'].append(int(round(seen['theta'] / 5)) if seen['ok'] else -1)
        cost = JP.heading_costs(seen['phi'])
        pat, srt = JP.pattern_of(seen['phi']), np.sort(cost)
        rec['unknown'].append(not JP.table_fits(perm[pat], eq[pat], cost) and bool((srt[1:] == srt[:-1]).any()))
        rec['drone'].append([env.drone.x, env.drone.y, float(np.asarray(env.drone.yaw).ravel()[0])])
        rec['vel'].append(np.concatenate([np.asarray(env.drone.velocity, dtype=np.float64).ravel(),
                                          np.asarray(env.drone.acceleration, dtype=np.float64).ravel()]))
        rec['sm'].append(env.state_machine)
        rec['fail'].append(env.fail_count)
        rec['flags'].append([info['collision_flag'], info['dead_lock_flag'], info['freezing_flag']])
        rec['done'].append(bool(done))
    buf = info['tracker_buffer']
    n = len(buf)
    gm = info['drone'].map.grid_map
    row = [info['flight_time'], float(gm.shape[0] * gm.shape[1] - np.sum(np.where(gm == 0, 1, 0))), n,
           float(np.array([len(t.ts) * 0.1 for t in buf]).sum() / n) if n else float('nan'),
           1 if info['state_machine'] == 1 else 0, 1 if info['collision_flag'] == 1 else 0, 1 if info['collision_flag'] == 2 else 0,
           info['freezing_flag'], info['dead_lock_flag'], info['state_machine']]
    dt = dict(g_active=np.uint8, plan_ok=np.uint8, choice=np.int32, sm=np.int32, fail=np.int32, flags=np.uint8, done=np.uint8,
              owl_left=np.int32, unknown=np.uint8)
    out = {'t_' + k: np.array(v, dtype=dt.get(k, np.float64)) for k, v in rec.items() if len(v)}
    out.update(cfg=np.array(json.dumps(kw)), N=np.array(N), row=np.array(row, dtype=np.float64))
    return out


_TIE = []


def tie_table():
    from drone2d_amd import jerk_plugin as JP
    if not _TIE:
        _TIE.append(JP.tie_table())
    return _TIE[0]


def search_deadlock():
    for m in DEADLOCK_IDS:
        d = record(dict(DEADLOCK, map_id=m))
        if d['row'][8] == 1:
            return m
    return None


def owl_facts(d):
    """(decisions with >= 2 active trackers, decisions with the drone at rest) of one recorded Owl world"""
    hold = int(d['t_owl_left'].max())
    decided = d['t_owl_left'] == hold
    return (int((decided & (d['t_g_active'].sum(1) >= 2)).sum()),
            int((decided & (d['t_g_drone'][:, 3] == 0) & (d['t_g_drone'][:, 4] == 0)).sum()))


def main():
    warnings.simplefilter('ignore')                      # Owl divides by the speed of a drone at rest
    worlds = list(WORLDS)
    if '--no-search' not in sys.argv:
        m = search_deadlock()
        print('dead-lock search:', f'map_id {m}' if m is not None else f'none in {DEADLOCK_IDS}')
        if m is not None:
            worlds.append(('deadlock', dict(DEADLOCK, map_id=m)))
    perm, eq = tie_table()
    out = {'names': np.array([w[0] for w in worlds]), 'tie_perm': perm, 'tie_eq': eq, 'numpy_version': np.array(np.__version__)}
    busy = rest = 0
    for i, (name, kw) in enumerate(worlds):
        d = record(kw)
        for k, v in d.items():
            out[f'w{i}_{k}'] = v
        print(name, 'N', int(d['N']), 'T', len(d['t_done']), 'failed plans', int((d['t_plan_ok'] == 0).sum()), 'row', d['row'].tolist())
        assert not d['t_unknown'].any(), f'{name}: a tie pattern outside the table'
        if kw['gaze_method'] in ('LookGoal', 'Oxford'):
            assert (d['t_action'] == 0).all(), f'{name}: a non-zero action'
        if kw['gaze_method'] == 'Owl':
            b, r = owl_facts(d)
            print('   Owl decisions with >= 2 active trackers:', b, ' with the drone at rest:', r)
            busy += b > 0
            rest += r > 0
    assert busy >= 3 and rest >= 2, (busy, rest)
    names = [w[0] for w in worlds]
    assert out[f'w{names.index("freezing")}_row'][7] == 1, 'the freezing world does not end by freezing'
    assert 'deadlock' in names, 'no dead-lock world'
    G.save('jerk_gaze_episodes', out)


if __name__ == '__main__':
    main()
