#!/usr/bin/env python3
"""Recorder of tests/golden/jerk_traces.npz: the reference env under --planner Jerk_Primitive, stepped through make_golden.py's
stubs with seeded random gaze actions.

Per world (prefix w<i>_): the parameters, the actions, and per step
  what plan() saw     p_drone (x, y, vx, vy, ax, ay), p_target, p_wall (the explored map's OCCUPIED cells, bit-packed), p_active,
                      p_radius (tracker.radius), p_mu (the trackers' latest mean)
  what plan() gave    plan_ok, wp (the appended waypoint: position, velocity, acceleration), choice (theta / 5 of the primitive it
                      took, -1 when it failed), phi_h
  the env afterwards  drone (x, y, yaw), vel (velocity, acceleration), sm, fail, flags, done
and the seconds per step the reference took on the recording machine.  With the traces: the tie table of the recording host's
np.argsort (drone2d_amd.jerk_plugin.tie_table) and its numpy version, so that a host with another numpy build replays the same
decisions.  What is stored is data; runs only where the reference is present.

The tie world: map ids 0 .. 199 of the default world are searched (the first TIE_STEPS steps each) for a step whose decision
depended on a tie -- the heading taken and the next one in numpy's order cost the same and are both free (tests/jerk_model.py says
so).  The first hit is recorded as world 'tie'; main() prints what the search found (under numpy 2.2.6: map_id 29, step 23, where phi_h
is 90, a tracker blocks every heading from 65 to 115, and 60 and 120 are both free: numpy's order takes 60).  The default world starts with phi_h exactly 90
and flies straight up, so every step of it ranks 35 tied pairs, but its best heading (90, untied) is almost always free.

Usage:  python tests/golden/make_jerk_golden.py [--no-search]
"""
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G   # noqa: E402  (installs the gym / pygame / cvxpy stubs, enters the reference's directory)
import jerk_model as M    # noqa: E402

WORLDS = [
    ('default40', dict(drone_max_speed=40, map_id=0), 50),
    ('default20', dict(drone_max_speed=20, map_id=1), 50),
    ('obstacle_map', dict(drone_max_speed=40, map_id=2, static_map='maps/obstacle_map.npy', agent_number=4), 100),
    ('var_cam2', dict(drone_max_speed=40, map_id=3, var_cam=2), 40),
    ('two_targets', dict(drone_max_speed=40, map_id=4, target_list=[[50, 130], [140, 130]]), 50),
    ('rvo', dict(drone_max_speed=40, map_id=5, motion_profile='RVO', agent_radius=15, agent_max_speed=20), 25),
]
TIE_STEPS = 40


def record(name, kw, T, stop_at_tie=False):
    p = G.make_params(planner='Jerk_Primitive', **kw)
    actions = np.random.RandomState(len(name) + 11).uniform(-1, 1, T)
    env = G.Drone2DEnv2(p)
    N = len(env.agents)
    planner = env.planner
    seen, rec = {}, {k: [] for k in ('p_drone', 'p_target', 'p_wall', 'p_active', 'p_radius', 'p_mu', 'plan_ok', 'wp', 'choice', 'phi_h',
                                     'drone', 'vel', 'sm', 'fail', 'flags', 'done', 'tie')}
    orig_plan, orig_prim = planner.plan, planner.generate_primitive

    def prim_wrap(p0, v0, a0, theta_h, v_max, delt_t):
        seen['theta'] = float(theta_h)
        return orig_prim(p0, v0, a0, theta_h, v_max, delt_t)

    def plan_wrap(drone, dt):
        trk = drone.trackers[:N]
        seen['in'] = dict(
            p_drone=np.concatenate([[drone.x, drone.y], np.asarray(drone.velocity, dtype=np.float64).ravel(),
                                    np.asarray(drone.acceleration, dtype=np.float64).ravel()]).astype(np.float64),
            p_target=np.asarray(planner.target[:2], dtype=np.float64).copy(),
            p_wall=np.packbits(drone.map.grid_map == 1),
            p_active=np.array([t.active for t in trk], dtype=np.uint8),
            p_radius=np.array([t.radius for t in trk], dtype=np.float64),
            p_mu=np.array([t.mu_upds[-1][:, 0] for t in trk], dtype=np.float64).reshape(N, 4))
        seen['grid'] = drone.map.grid_map.copy()
        ok = orig_plan(drone, dt)
        tr = planner.trajectory
        seen['ok'] = bool(ok)
        seen['wp'] = np.concatenate([np.asarray(tr.positions[0], dtype=np.float64), np.asarray(tr.velocities[0], dtype=np.float64),
                                     np.asarray(tr.accelerations[0], dtype=np.float64)]) if len(tr) else np.zeros(6)
        return ok
    planner.plan, planner.generate_primitive = plan_wrap, prim_wrap
    t0 = time.perf_counter()
    for t in range(T):
        _, _, done, info = env.step(float(actions[t]))
        i = seen['in']
        for k, v in i.items():
            rec[k].append(v)
        rec['plan_ok'].append(seen['ok'])
        rec['wp'].append(seen['wp'])
        rec['choice'].append(int(round(seen['theta'] / 5)) if seen['ok'] else -1)
        rec['phi_h'].append(math.degrees(math.atan2(i['p_target'][1] - i['p_drone'][1], i['p_target'][0] - i['p_drone'][0])))
        rec['drone'].append([env.drone.x, env.drone.y, float(np.asarray(env.drone.yaw).ravel()[0])])
        rec['vel'].append(np.concatenate([np.asarray(env.drone.velocity, dtype=np.float64).ravel(),
                                          np.asarray(env.drone.acceleration, dtype=np.float64).ravel()]))
        rec['sm'].append(env.state_machine)
        rec['fail'].append(env.fail_count)
        rec['flags'].append([info['collision_flag'], info['dead_lock_flag'], info['freezing_flag']])
        rec['done'].append(bool(done))
        scene = dict(drone=tuple(i['p_drone']), target=tuple(i['p_target']), dmap=seen['grid'],
                     trackers=[(i['p_mu'][k], i['p_radius'][k]) for k in range(N) if i['p_active'][k]], scale=p.map_scale,
                     map_size=tuple(p.map_size), drone_radius=p.drone_radius, var_cam=p.var_cam, v_max=p.drone_max_speed, dt=p.dt)
        rec['tie'].append(bool(M.plan(scene)['tie']))
        if done or (stop_at_tie and rec['tie'][-1]):
            break
    seconds = (time.perf_counter() - t0) / len(rec['done'])
    dt = dict(plan_ok=np.uint8, choice=np.int32, sm=np.int32, fail=np.int32, flags=np.uint8, done=np.uint8, tie=np.uint8)
    d = {'t_' + k: np.array(v, dtype=dt.get(k, None)) for k, v in rec.items()}
    d.update(actions=actions[:len(rec['done'])], cfg=np.array(json.dumps(kw)), N=np.array(N), ref_seconds_per_step=np.array(seconds))
    return d


def search_tie():
    for m in range(200):
        d = record('tie', dict(drone_max_speed=40, map_id=m), TIE_STEPS, stop_at_tie=True)
        if d['t_tie'].any():
            return m, len(d['t_tie'])
    return None, 0


def main():
    from drone2d_amd import jerk_plugin as JP
    worlds = list(WORLDS)
    if '--no-search' not in sys.argv:
        m, steps = search_tie()
        print('tie search:', f'map_id {m}, step {steps - 1}' if m is not None else 'none in 200 seeds')
        if m is not None:
            worlds.append(('tie', dict(drone_max_speed=40, map_id=m), min(steps + 3, TIE_STEPS)))
    perm, eq = JP.tie_table()
    out = {'names': np.array([w[0] for w in worlds]), 'tie_perm': perm, 'tie_eq': eq, 'numpy_version': np.array(np.__version__)}
    for i, (name, kw, T) in enumerate(worlds):
        for k, v in record(name, kw, T).items():
            out[f'w{i}_{k}'] = v
        print(name, 'N', int(out[f'w{i}_N']), 'T', len(out[f'w{i}_t_done']), 'failed plans', int((out[f'w{i}_t_plan_ok'] == 0).sum()),
              'choices', sorted(set(out[f'w{i}_t_choice'].tolist())), 'ties', int(out[f'w{i}_t_tie'].sum()),
              f"{float(out[f'w{i}_ref_seconds_per_step']):.4f} s/step")
    G.save('jerk_traces', out)


if __name__ == '__main__':
    main()
