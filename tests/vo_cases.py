"""Shared inputs of the velocity-obstacle metric's tests: the recorded fixture, the seeded host worlds, the adversarial world and
the Python model's results (computed once per process and argument set)."""
import functools
import json
import os

import numpy as np

import drone2d_amd as pkg
from drone2d_amd import host_init, metrics

import vo_model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vo_feasibility.npz')


@functools.lru_cache(maxsize=None)
def fixture():
    """[(index, dict of agent_pos, agent_pref, agent_radius, rates, collided, mean, density, ref_seconds)] of the three settings"""
    z = np.load(GOLD)
    out = []
    for i in range(int(z['n'])):
        out.append((json.loads(str(z[f's{i}_index'])),
                    {k: z[f's{i}_{k}'] for k in ('agent_pos', 'agent_pref', 'agent_radius', 'rates', 'collided', 'mean', 'density',
                                                 'ref_seconds')}))
    return out


def fixture_agents(rec):
    """the recorded agents in the state's layout [6, N]"""
    r = rec['agent_radius']
    return np.stack([rec['agent_pos'][:, 0], rec['agent_pos'][:, 1], rec['agent_pref'][:, 0], rec['agent_pref'][:, 1], r, r ** 2])


def world_of(params):
    return host_init.init_world(pkg.with_defaults(params))


def vo_params(agent_number, agent_radius=10, agent_max_speed=40, map_id=0, **kw):
    """a world of the metric's kind (drone_radius=0, NoMove) with free map settings"""
    p = pkg.Params(agent_number=agent_number, agent_radius=agent_radius, agent_max_speed=agent_max_speed, map_id=map_id,
                   gaze_method='NoControl', planner='NoMove', drone_radius=0, debug=True, **kw)
    p.render = False
    return p


def positions_of(params, step):
    xs, ys = metrics.vo_positions(params, step)
    return np.array([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def candidates():
    return metrics.vo_candidates()


@functools.lru_cache(maxsize=None)
def fixture_model(i, step):
    """the model on fixture world i at `step` px between positions"""
    index, rec = fixture()[i]
    return vo_model.vo_world(fixture_agents(rec), positions_of(metrics._params(index), step), candidates())


ADV_POS = np.array([[10.0, 10.0], [250.0, 250.0], [460.0, 460.0]])


@functools.lru_cache(maxsize=None)
def adversarial():
    """One world of N = 70 agents [6, N] for ADV_POS and the default candidates:
      0  at (250, 262), r = 7: distance rA + r from (250, 250) exactly -- not a collision, half angle asin(1.0)
      1  at (200, 250): due west of (250, 250), theta_BA = pi, a cone across the +-pi cut (in_between's first wrap branch)
      2  at (262, 250.001), r = 7: almost touching, half angle > 1.57 around theta_BA ~ 0 (the second wrap branch)
      3  pref_velocity = candidate 123's bits: atan2(0.0, 0.0)
      4, 5  share candidate 317's vy only, vx beyond / short of it: atan2(0.0, x) with x of both signs
      6  contains (460, 460); so does the LAST agent, 69 (the reference stops at 6 and never sees it)
    the rest random, clear of each other, of these and of the three positions."""
    rng = np.random.RandomState(20)
    cand = candidates()
    N = 70
    x, y, r = np.zeros(N), np.zeros(N), np.zeros(N)
    ang = rng.uniform(0, 2 * np.pi, N)
    vx, vy = -40 * np.cos(ang), -40 * np.sin(ang)
    fixed = {0: (250.0, 262.0, 7.0), 1: (200.0, 250.0, 9.0), 2: (262.0, 250.001, 7.0), 6: (458.0, 461.0, 12.0), 69: (465.0, 455.0, 10.0)}
    for k, v in fixed.items():
        x[k], y[k], r[k] = v
    placed = list(fixed)
    for k in range(N):
        if k in fixed:
            continue
        while True:
            cx, cy, cr = rng.uniform(20, 480), rng.uniform(20, 480), rng.uniform(4, 9)
            if all(np.hypot(cx - x[q], cy - y[q]) > cr + r[q] + 1 for q in placed) and \
                    all(np.hypot(cx - px, cy - py) > cr + 5 + 1 for px, py in ADV_POS):
                break
        x[k], y[k], r[k] = cx, cy, cr
        placed.append(k)
    vx[3], vy[3] = cand[123]
    vx[4], vy[4] = cand[317, 0] + 3.0, cand[317, 1]
    vx[5], vy[5] = cand[317, 0] - 3.0, cand[317, 1]
    return np.stack([x, y, vx, vy, r, r ** 2])


@functools.lru_cache(maxsize=None)
def adversarial_model():
    return vo_model.vo_world(adversarial(), ADV_POS, candidates())
