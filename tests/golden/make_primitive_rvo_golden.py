#!/usr/bin/env python3
"""Recorder of tests/golden/primitive_rvo_episodes.npz: whole episodes of the reference under --planner Primitive --motion_profile RVO,
driven as experiment.py:65-70 drives them -- policy.__init__(policy, params); while not done: a = policy.plan(policy, env.info);
env.step(a) -- through make_golden.py's stubs.

Per world (prefix w<i>_): the parameters, N, the CSV row of experiment.py:73-103 (`row`: flight time, grid discovered, agents tracked,
mean tracked time, success, static collision, dynamic collision, freezing, dead lock, state machine), `ref_s_per_step` (the wall time
of the reference's own loop on the recording host, per step of this one env) and per step
  the policy's answer   action; for Owl: owl_U (U_list after the call), owl_left (len(Owl.u)), owl_rate (the yaw rate it holds)
  what plan() gave      plan_ok, wp_valid, wp (the head waypoint step_pos consumes: position, velocity, acceleration), replanned
                        (replan_check threw a non-empty trajectory away)
  the env afterwards    traj_len (len(trajectory)), drone (x, y, yaw), vel (velocity, acceleration), sm, fail, flags, done,
                        agent_pos, agent_vel (every agent's position and the velocity RVO_update gave it)
What is stored is data; runs only where the reference is present.

Usage:  python tests/golden/make_primitive_rvo_golden.py
"""
import json
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)

BASE = dict(motion_profile='RVO', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40)
WORLDS = [
    ('lookahead_success', dict(BASE, gaze_method='LookAhead', map_id=0, max_flight_time=40)),
    ('lookahead_collision', dict(BASE, gaze_method='LookAhead', map_id=1, max_flight_time=40)),
    ('lookahead_deadlock', dict(BASE, gaze_method='LookAhead', map_id=3, max_flight_time=40)),
    ('oxford_freezing', dict(BASE, gaze_method='Oxford', map_id=1, max_flight_time=12)),
    ('owl_pillars', dict(BASE, gaze_method='Owl', map_id=2, max_flight_time=4, pillar_number=3)),
    ('lookgoal_var_cam2', dict(BASE, gaze_method='LookGoal', map_id=4, max_flight_time=4, var_cam=2)),
    ('lookahead_drone20', dict(BASE, gaze_method='LookAhead', map_id=5, max_flight_time=4, drone_max_speed=20)),
    ('rotating', dict(BASE, gaze_method='Rotating', map_id=6, max_flight_time=3)),
    ('nocontrol', dict(BASE, gaze_method='NoControl', map_id=7, max_flight_time=3)),
]


def record(kw):
    p = G.make_params(planner='Primitive', **kw)
    if p.gaze_method == 'NoControl':
        p.drone_view_range = 360                                   # experiment.py:28-29
    env = G.Drone2DEnv2(p)
    pol = getattr(G.yaw_planner, p.gaze_method)
    pol.__init__(pol, p)
    N = len(env.agents)
    planner = env.planner
    seen = {}
    orig_plan, orig_check = planner.plan, planner.replan_check

    def check_wrap(drone):
        before = len(planner.trajectory)
        out = orig_check(drone)
        seen['replanned'] = bool(out[0]) and before > 0
        return out

    def plan_wrap(drone, dt):
        seen['ok'] = bool(orig_plan(drone, dt))
        tr = planner.trajectory
        seen['n'] = len(tr)
        seen['wp'] = np.zeros(6)
        if len(tr):
            seen['wp'] = np.concatenate([np.asarray(x[0], dtype=np.float64).ravel() for x in (tr.positions, tr.velocities, tr.accelerations)])
        return seen['ok']
    planner.plan, planner.replan_check = plan_wrap, check_wrap
    keys = ('action', 'owl_U', 'owl_left', 'owl_rate', 'plan_ok', 'wp_valid', 'wp', 'replanned', 'traj_len', 'drone', 'vel', 'sm', 'fail',
            'flags', 'done', 'agent_pos', 'agent_vel')
    rec = {k: [] for k in keys}
    done, info, held = False, None, 0.0
    t0 = time.perf_counter()
    while not done:
        a = pol.plan(pol, env.info)
        a = 0.0 if a is None else float(a)
        rec['action'].append(a)
        if p.gaze_method == 'Owl':
            if len(pol.u):
                held = float(pol.u[-1])
            rec['owl_U'].append(np.array(pol.U_list, dtype=np.float64))
            rec['owl_left'].append(len(pol.u))
            rec['owl_rate'].append(held)
        _, _, done, info = env.step(a)
        rec['plan_ok'].append(seen['ok'])
        rec['wp_valid'].append(seen['n'] > 0)
        rec['wp'].append(seen['wp'])
        rec['replanned'].append(seen['replanned'])
        rec['traj_len'].append(len(planner.trajectory))
        rec['drone'].append([env.drone.x, env.drone.y, float(np.asarray(env.drone.yaw).ravel()[0])])
        rec['vel'].append(np.concatenate([np.asarray(env.drone.velocity, dtype=np.float64).ravel(),
                                          np.asarray(env.drone.acceleration, dtype=np.float64).ravel()]))
        rec['sm'].append(env.state_machine)
        rec['fail'].append(env.fail_count)
        rec['flags'].append([info['collision_flag'], info['dead_lock_flag'], info['freezing_flag']])
        rec['done'].append(bool(done))
        rec['agent_pos'].append(np.array([ag.position for ag in env.agents], dtype=np.float64).reshape(N, 2))
        rec['agent_vel'].append(np.array([ag.velocity for ag in env.agents], dtype=np.float64).reshape(N, 2))
    wall = time.perf_counter() - t0
    buf = info['tracker_buffer']
    n = len(buf)
    gm = info['drone'].map.grid_map
    row = [info['flight_time'], float(gm.shape[0] * gm.shape[1] - np.sum(np.where(gm == 0, 1, 0))), n,
           float(np.array([len(t.ts) * 0.1 for t in buf]).sum() / n) if n else float('nan'),
           1 if info['state_machine'] == 1 else 0, 1 if info['collision_flag'] == 1 else 0, 1 if info['collision_flag'] == 2 else 0,
           info['freezing_flag'], info['dead_lock_flag'], info['state_machine']]
    dt = dict(plan_ok=np.uint8, wp_valid=np.uint8, replanned=np.uint8, traj_len=np.int32, sm=np.int32, fail=np.int32, flags=np.uint8,
              done=np.uint8, owl_left=np.int32)
    out = {'t_' + k: np.array(v, dtype=dt.get(k, np.float64)) for k, v in rec.items() if len(v)}
    out.update(cfg=np.array(json.dumps(kw)), N=np.array(N), row=np.array(row, dtype=np.float64),
               ref_s_per_step=np.array(wall / len(rec['done'])))
    return out


def main():
    warnings.simplefilter('ignore')                      # Owl divides by the speed of a drone at rest
    out = {'names': np.array([w[0] for w in WORLDS]), 'numpy_version': np.array(np.__version__)}
    ends, failed, replanned = set(), 0, 0
    for i, (name, kw) in enumerate(WORLDS):
        d = record(kw)
        for k, v in d.items():
            out[f'w{i}_{k}'] = v
        r = d['row']
        ends |= {e for e, on in (('success', r[4]), ('dynamic collision', r[6]), ('freezing', r[7]), ('dead lock', r[8])) if on}
        failed += int((d['t_plan_ok'] == 0).sum()) > 0
        replanned += int(d['t_replanned'].sum()) > 0
        print(name, 'N', int(d['N']), 'T', len(d['t_done']), 'failed plans', int((d['t_plan_ok'] == 0).sum()), 'replans',
              int(d['t_replanned'].sum()), f'{float(d["ref_s_per_step"]) * 1e3:.1f} ms/step', 'row', r.tolist())
    assert ends == {'success', 'dynamic collision', 'freezing', 'dead lock'}, ends
    assert failed >= 1, 'no world with a failed plan'
    assert replanned >= 1, 'no trajectory replaced by a replan'
    G.save('primitive_rvo_episodes', out)


if __name__ == '__main__':
    main()
