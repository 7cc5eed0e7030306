"""Scalar Python model of the Jerk_Primitive planner (include/d2d_jerk.h), in this project's own words, with numpy live: cos, sin,
scalar `**`, numpy's norm of a 2-vector and `np.argsort` are evaluated here as the reference evaluates them, not read from the
tables the device takes.  The CPU tests compare it with the recorded reference (tests/golden/jerk_traces.npz) and with the host
build of csrc/jerk/d2d_jerk.h; the GPU tests compare the kernel with it.

One decision = `plan(scene)`.  A scene is a dict:
  drone     (x, y, vx, vy, ax, ay)            target  (gx, gy)
  dmap      uint8 [W, H], the explored map     trackers  list of (mu[4], radius) of the ACTIVE trackers, in tracker order
  scale, map_size (W_px, H_px), drone_radius, var_cam, v_max, dt
"""
import math

import numpy as np
from numpy.linalg import norm

OCCUPIED = 1
N_THETA = 72
END_DISTANCE = 30


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def goal_direction(scene):
    x, y = scene['drone'][0], scene['drone'][1]
    to_goal = np.array(scene['target'], dtype=np.float64) - np.array([x, y])
    return math.degrees(math.atan2(to_goal[1], to_goal[0]))


def costs(phi_h):
    """[72] squared angular distance of every heading to the goal direction"""
    goal = phi_h % 360
    out = np.zeros(N_THETA)
    for i, theta in enumerate(np.arange(0, 360, 5)):
        apart = abs(theta % 360 - goal)
        out[i] = (apart if apart <= 180 else 360 - apart) ** 2
    return out


def cell_value(scene, x, y):
    """the map's answer for a point in pixels: occupied outside the map"""
    W_px, H_px = scene['map_size']
    if x >= W_px or x < 0 or y >= H_px or y < 0:
        return OCCUPIED
    return scene['dmap'][int(x // scene['scale']), int(y // scene['scale'])]


def sample_free(scene, position, t):
    if np.isnan(position).any():
        return False
    reach = scene['drone_radius'] + 10
    for dx, dy in ((-reach, 0), (0, 0), (reach, 0), (0, -reach), (0, reach)):
        if cell_value(scene, position[0] + dx, position[1] + dy) == OCCUPIED:
            return False
    for mu, radius in scene['trackers']:
        mu = np.asarray(mu, dtype=np.float64)
        predicted = mu[:2] + t * mu[2:4]
        if norm(position - predicted) <= scene['drone_radius'] + radius + 5 + scene['var_cam']:
            return False
    return True


def primitive(scene, theta):
    """positions, velocities, accelerations [times, 2] and sample times of the jerk-optimal primitive of heading theta (degrees)"""
    p0 = np.array(scene['drone'][0:2], dtype=np.float64)
    v0 = np.array(scene['drone'][2:4], dtype=np.float64)
    a0 = np.array(scene['drone'][4:6], dtype=np.float64)
    v_max, dt = scene['v_max'], scene['dt']
    step = np.array([END_DISTANCE * np.cos(math.radians(theta)), END_DISTANCE * np.sin(math.radians(theta))])
    pf = p0 + step
    to_goal = np.array(scene['target'], dtype=np.float64) - pf
    with np.errstate(all='ignore'):
        vf = (0.5 * v_max / norm(to_goal)) * to_goal
    T = 1.2 * norm(step) / norm(v_max)
    T = T if T >= 0.5 else 0.5
    times = int(np.floor(T / dt))
    ts = np.arange(dt, times * dt + dt, dt)
    p, v, a = np.zeros((times, 2)), np.zeros((times, 2)), np.zeros((times, 2))
    for ax in range(2):
        da = 0 - a0[ax]
        dv = vf[ax] - v0[ax] - a0[ax] * T
        dp = pf[ax] - p0[ax] - v0[ax] * T - 0.5 * a0[ax] * T ** 2
        alpha = da * 60 / T ** 3 - dv * 360 / T ** 4 + dp * 720 / T ** 5
        beta = -da * 24 / T ** 2 + dv * 168 / T ** 3 - dp * 360 / T ** 4
        gamma = da * 3 / T - dv * 24 / T ** 2 + dp * 60 / T ** 3
        for j in range(times):
            tt = ts[j]
            p[j, ax] = alpha / 120 * tt ** 5 + beta / 24 * tt ** 4 + gamma / 6 * tt ** 3 + a0[ax] / 2 * tt ** 2 + v0[ax] * tt + p0[ax]
            v[j, ax] = alpha / 24 * tt ** 4 + beta / 6 * tt ** 3 + gamma / 2 * tt ** 2 + a0[ax] * tt + v0[ax]
            a[j, ax] = alpha / 6 * tt ** 3 + beta / 2 * tt ** 2 + gamma * tt + a0[ax]
    return p, v, a, ts[:times]


def primitive_free(scene, theta):
    p, v, a, ts = primitive(scene, theta)
    return all(sample_free(scene, p[j], ts[j]) for j in range(len(ts))), (p, v, a)


def plan(scene, argsort=np.argsort, order=None):
    """the decision: dict(plan_ok, choice (heading index or -1), wp [6], phi_h, tie, tested, order).  `order`: a ranking of the 72
    headings to walk instead of argsort's (the device's table row)."""
    phi_h = goal_direction(scene)
    cost = costs(phi_h)
    if order is None:
        order = np.asarray(argsort(cost))
    out = dict(plan_ok=0, choice=-1, wp=np.zeros(6), phi_h=phi_h, tie=False, tested=0, order=np.asarray(order), cost=cost)
    for rank, i in enumerate(order):
        free, (p, v, a) = primitive_free(scene, 5.0 * i)
        out['tested'] += 1
        if not free:
            continue
        out.update(plan_ok=1, choice=int(i), wp=np.concatenate([p[0], v[0], a[0]]))
        # the decision depended on a tie: the next heading in the order costs the same and is free as well
        if rank + 1 < N_THETA and cost[order[rank + 1]] == cost[i]:
            out['tie'] = primitive_free(scene, 5.0 * order[rank + 1])[0]
        break
    return out


def step_trackers(radius, prev, active, agent_radius):
    """the tracker-radius bookkeeping of one env, in place: a tracker that was active and is not any more gets agent_radius back"""
    for k in range(len(radius)):
        if prev[k] and not active[k]:
            radius[k] = agent_radius
        prev[k] = 1 if active[k] else 0
