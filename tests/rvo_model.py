"""Scalar Python model of the RVO motion profile (include/d2d_rvo.h), in this project's own words: math.*, numpy's norm of a
2-vector, the velocity and the preferred velocity of an agent as separate values.  The CPU tests compare it with the recorded
reference (tests/golden/rvo_traces.npz) and with the host build of csrc/rvo/d2d_rvo.h; the GPU tests compare the kernels with it.

One decision = `decide`: the cones of the other agents and of the pillars, the candidate velocities, and the choice among them.
One env-step = `step_world`: every decision from the positions and velocities of before the step, then every agent's move."""
import math

import numpy as np
from numpy.linalg import norm

from vo_model import in_between

A_PX, A_PY, A_VX, A_VY, A_R, A_R2 = range(6)
N_THETA = 32                       # len(np.arange(0, 2 * 3.14, 0.2))
THETAS = [i * 0.2 for i in range(N_THETA)]
COS_T = [math.cos(t) for t in THETAS]
SIN_T = [math.sin(t) for t in THETAS]
WT = 0.2
COS30, SIN30 = math.cos(math.pi / 6), math.sin(math.pi / 6)

# what a decision took (the `kind` of decide)
PREF, GRID, NO_SUITABLE = 0, 1, 2


def arange_replay(norm_v):
    """np.arange(0.02, norm_v + 0.02, norm_v / 5.0) by numpy's rule: the length is ceil((stop - start) / step), element i is
    start + i * ((start + step) - start).  A list of floats."""
    norm_v = float(norm_v)
    start, stop, step = 0.02, norm_v + 0.02, norm_v / 5.0
    val = (stop - start) / step
    n = int(math.ceil(val)) if val > 0 else 0
    delta = (start + step) - start
    return [start + i * delta for i in range(n)]


def seq_min(keys):
    """Python's min(range(len(keys)), key=keys.__getitem__): the first minimum; a NaN wins only from position 0"""
    best = 0
    for i in range(1, len(keys)):
        if keys[i] < keys[best]:
            best = i
    return best


def parallel_argmin(keys, lanes=64):
    """The device's rule, which has to equal seq_min: position 0 if its key is a NaN; otherwise the smallest non-NaN key, the lowest
    index among equals.  Evaluated the way the wave does: each lane over its strided share, then a tree over the lanes."""
    if keys[0] != keys[0]:
        return 0
    part = []
    for lane in range(lanes):
        bk, bi = math.inf, 1 << 30
        for i in range(lane, len(keys), lanes):
            k = keys[i]
            if k == k and (k < bk or (k == bk and i < bi)):
                bk, bi = k, i
        part.append((bk, bi))
    w = lanes
    while w > 1:
        w //= 2
        for lane in range(w):
            (ak, ai), (ck, ci) = part[lane], part[lane + w]
            if ck < ak or (ck == ak and ci < ai):
                part[lane] = (ck, ci)
    return part[0][1]


def norm2(x, y):
    return float(norm(np.array([x, y], dtype=np.float64)))


def cones_of(i, pos, vel, rob_rad, pillars):
    """the cones of agent i: [apex x, apex y, theta_right, theta_left, dist, rad] per other agent, then per pillar"""
    pax, pay = float(pos[i][0]), float(pos[i][1])
    vax, vay = float(vel[i][0]), float(vel[i][1])
    out = []
    for j in range(len(pos)):
        if j == i:
            continue
        pbx, pby = float(pos[j][0]), float(pos[j][1])
        vbx, vby = float(vel[j][0]), float(vel[j][1])
        apex = (pax + 0.5 * (vbx + vax), pay + 0.5 * (vby + vay))
        dist = norm2(pax - pbx, pay - pby)
        theta = math.atan2(pby - pay, pbx - pax)
        rad = 2 * rob_rad
        if rad > dist:
            dist = rad
        half = math.asin(rad / dist)
        le, ri = theta + half, theta - half
        out.append([apex[0], apex[1], math.atan2(math.sin(ri), math.cos(ri)), math.atan2(math.sin(le), math.cos(le)), dist, rad])
    for hole in pillars:
        pbx, pby = float(hole[0]), float(hole[1])
        apex = (pax + 0.0, pay + 0.0)
        dist = norm2(pax - pbx, pay - pby)
        theta = math.atan2(pby - pay, pbx - pax)
        rad = float(hole[2]) * 1.5 + rob_rad
        if rad > dist:
            dist = rad
        half = math.asin(rad / dist)
        le, ri = theta + half, theta - half
        out.append([apex[0], apex[1], math.atan2(math.sin(ri), math.cos(ri)), math.atan2(math.sin(le), math.cos(le)), dist, rad])
    return out


def candidates_of(prefx, prefy):
    """theta-major, then rad, the preferred velocity last"""
    rads = arange_replay(norm2(prefx, prefy))
    cand = [(r * COS_T[t], r * SIN_T[t]) for t in range(N_THETA) for r in rads]
    cand.append((prefx, prefy))
    return cand


def _div(a, b):
    """numpy's float64 division: 0 / 0 is a NaN, x / 0 an infinity"""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a)
    return a / b


def decide(i, pos, vel, pref, rob_rad, pillars, argmin=seq_min):
    """-> (vx, vy, kind, index of the candidate, number of candidates, counts: candidates inside a pillar's cone, divisions by
    norm(dif) == 0, NaN keys, clamped cones)"""
    pax, pay = float(pos[i][0]), float(pos[i][1])
    prefx, prefy = float(pref[i][0]), float(pref[i][1])
    cones = cones_of(i, pos, vel, rob_rad, pillars)
    cand = candidates_of(prefx, prefy)
    inside = []                               # per candidate: [(cone, theta_dif, dif x, dif y)] of the cones it lies in
    for (cx, cy) in cand:
        hits = []
        for cn in cones:
            dx, dy = cx + pax - cn[0], cy + pay - cn[1]
            td = math.atan2(dy, dx)
            if in_between(cn[2], td, cn[3]):
                hits.append((cn, td, dx, dy))
        inside.append(hits)
    dist_pref = [norm2(cx - prefx, cy - prefy) for (cx, cy) in cand]
    suitable = [c for c in range(len(cand)) if not inside[c]]
    if suitable:
        c = suitable[argmin([dist_pref[k] for k in suitable])]
        kind = PREF if c == len(cand) - 1 else GRID
    else:
        keys = []
        for c in range(len(cand)):
            tc = []
            for (cn, td, dx, dy) in inside[c]:
                dist, rad = cn[4], cn[5]
                small = abs(td - 0.5 * (cn[3] + cn[2]))
                s = abs(dist * math.sin(small))
                if s >= rad:
                    rad = s
                big = math.asin(s / rad)
                tg = abs(dist * math.cos(small)) - abs(rad * math.cos(big))
                if tg < 0:
                    tg = 0.0
                tc.append(_div(tg, norm2(dx, dy)))
            keys.append(WT / (tc[seq_min(tc)] + 0.001) + dist_pref[c])
        c = argmin(keys)
        kind = NO_SUITABLE
    n_agents = len(pos) - 1                   # the cones behind them are the pillars'
    extra = dict(
        on_apex=sum(dx == 0 and dy == 0 for hits in inside for (_, _, dx, dy) in hits) if kind == NO_SUITABLE else 0,
        nan_keys=sum(k != k for k in keys) if kind == NO_SUITABLE else 0,
        in_pillar_cone=sum(any(cn is pc for pc in cones[n_agents:] for (cn, _, _, _) in hits) for hits in inside),
        clamped=sum(cn[4] == cn[5] for cn in cones))      # cones whose dist was raised to rad: an overlap
    return cand[c][0], cand[c][1], kind, c, len(cand), extra


def velocities(pos, vel, pref, radius, pillars, argmin=seq_min, kinds=None):
    """RVO_update: every agent's new velocity from the positions and velocities of before the call; [N, 2]"""
    N = len(pos)
    out = np.zeros((N, 2))
    if N == 0:
        return out
    rob_rad = float(radius[0]) + 0.01
    for i in range(N):
        vx, vy, kind, c, C, extra = decide(i, pos, vel, pref, rob_rad, pillars, argmin)
        out[i] = (vx, vy)
        if kinds is not None:
            kinds.append((kind, c, C, extra))
    return out


def agent_step(px, py, vx, vy, prefx, prefy, r, W_px, H_px, scale, dt):
    """Agent.step with velocity and pref_velocity as separate values -> (px, py, prefx, prefy, rotated, flipped)"""
    nx, ny = px + vx * dt, py + vy * dt
    rotated = norm2(vx, vy) <= 5
    if rotated:
        m = np.array([[COS30, math.sin(-math.pi / 6)], [SIN30, COS30]]) @ np.array([prefx, prefy]).reshape(-1, 1)
        prefx, prefy = float(m[0, 0]), float(m[1, 0])
    before = (prefx, prefy)
    if nx < scale + r:
        prefx = abs(prefx)
    elif nx > W_px - scale - r:
        prefx = -abs(prefx)
    if ny < scale + r:
        prefy = abs(prefy)
    elif ny > H_px - scale - r:
        prefy = -abs(prefy)
    flipped = (math.copysign(1, prefx), math.copysign(1, prefy)) != (math.copysign(1, before[0]), math.copysign(1, before[1]))
    return nx, ny, prefx, prefy, rotated, flipped


def step_world(pos, vel, pref, radius, pillars, map_size=(500, 500), scale=10, dt=0.1, argmin=seq_min, events=None):
    """One env-step of the agents -> (pos, vel, pref) [N, 2] each.  events: a dict that counts what happened."""
    N = len(pos)
    kinds = []
    nvel = velocities(pos, vel, pref, radius, pillars, argmin, kinds)
    npos, npref = np.zeros((N, 2)), np.zeros((N, 2))
    for i in range(N):
        px, py, fx, fy, rot, flip = agent_step(float(pos[i][0]), float(pos[i][1]), nvel[i, 0], nvel[i, 1], float(pref[i][0]),
                                               float(pref[i][1]), float(radius[i]), map_size[0], map_size[1], scale, dt)
        npos[i], npref[i] = (px, py), (fx, fy)
        if events is not None:
            events['rotated'] = events.get('rotated', 0) + rot
            events['flipped'] = events.get('flipped', 0) + flip
    if events is not None:
        for kind, c, C, extra in kinds:
            for k, v in extra.items():
                events[k] = events.get(k, 0) + v
            events[('kind', kind)] = events.get(('kind', kind), 0) + 1
            events[('C', C)] = events.get(('C', C), 0) + 1
    return npos, nvel, npref


def planes(pos, pref, radius):
    """the state's agents [6, N] of one env"""
    N = len(pos)
    a = np.zeros((6, N))
    if N:
        a[A_PX], a[A_PY] = np.asarray(pos, dtype=np.float64).T
        a[A_VX], a[A_VY] = np.asarray(pref, dtype=np.float64).T
        a[A_R] = radius
        a[A_R2] = np.asarray(radius, dtype=np.float64) ** 2
    return a


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
