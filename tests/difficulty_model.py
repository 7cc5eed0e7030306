"""Scalar Python model of the traversability and survival-fit metrics (include/d2d_metrics.h) from a host world, in this project's
own words.  The CPU tests compare it with the recorded reference (tests/golden/difficulty_tables.npz) and with the host build of
csrc/metrics/d2d_difficulty.h; the GPU tests compare the kernels with it."""
import math

import numpy as np
from numpy.linalg import norm

A_PX, A_PY, A_VX, A_VY, A_R, A_R2 = range(6)
UNOCCUPIED = 2
DIRECTIONS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))     # N, NE, E, SE, S, SW, W, NW on grid[i][j]
TURN = np.array([[np.cos(np.pi / 6), np.sin(-np.pi / 6)], [np.sin(np.pi / 6), np.cos(np.pi / 6)]])


# ---- traversability

def trav_steps(grid, starts):
    """grid [W, H], starts: S pairs (i, j) inside it -> int32 [S, 8]: the cells walked per direction while the next one is inside
    the grid and UNOCCUPIED, or -1 in all eight where the start cell is not UNOCCUPIED"""
    g = np.asarray(grid).tolist()
    W, H = len(g), len(g[0])
    out = np.full((len(starts), 8), -1, dtype=np.int32)
    for s, (i0, j0) in enumerate(starts):
        if g[i0][j0] != UNOCCUPIED:
            continue
        for d, (di, dj) in enumerate(DIRECTIONS):
            i, j, n = i0 + di, j0 + dj, 0
            while 0 <= i < W and 0 <= j < H and g[i][j] == UNOCCUPIED:
                i, j, n = i + di, j + dj, n + 1
            out[s, d] = n
    return out


def trav_distances(row):
    """the eight distances of one open start from its step counts: a straight step adds the int 1, a diagonal one math.sqrt(2),
    one at a time"""
    out = []
    for d, k in enumerate(row):
        dist = 0
        for _ in range(int(k)):
            dist += math.sqrt(2) if d % 2 else 1
        out.append(dist)
    return out


def trav_world(grid, starts):
    """dict of steps [S, 8] int32, distances [S, 8] (-1 where the start is occupied), values [S] (np.mean of the eight, 0 where
    occupied) and metric (their running sum in start order over S)"""
    steps = trav_steps(grid, starts)
    distances = np.full(steps.shape, -1.0)
    values = []
    for s, row in enumerate(steps.tolist()):
        if row[0] < 0:
            values.append(0)
            continue
        eight = trav_distances(row)
        distances[s] = eight
        values.append(np.mean(eight))
    total = 0
    for v in values:
        total += v
    return dict(steps=steps, distances=distances, values=np.array(values, dtype=np.float64), metric=np.float64(total / len(values)))


# ---- survival fit

def agent_update(px, py, vx, vy, r, W_px, H_px, scale, dt):
    """One step of one agent under the constant-velocity model; (vx, vy) is pref_velocity.  The agent moves by pref_velocity as the
    bounces leave it -- except in a step whose stuck-agent turn replaces pref_velocity: that step moves by the value before it."""
    nx, ny = px + vx * dt, py + vy * dt
    moved_by = None
    if norm(np.array([vx, vy])) <= 5:
        moved_by = (vx, vy)
        turned = TURN @ np.array([[vx], [vy]])
        vx, vy = turned[0, 0], turned[1, 0]
    if nx < scale + r:
        vx = abs(vx)
    elif nx > W_px - scale - r:
        vx = -abs(vx)
    if ny < scale + r:
        vy = abs(vy)
    elif ny > H_px - scale - r:
        vy = -abs(vy)
    ux, uy = moved_by if moved_by is not None else (vx, vy)
    return px + ux * dt, py + uy * dt, vx, vy


def agents_update(agents, W_px, H_px, scale, dt):
    out = np.array(agents, dtype=np.float64)
    for j in range(out.shape[1]):
        out[:4, j] = agent_update(*out[:5, j].tolist(), W_px, H_px, scale, dt)
    return out


def hits(agents, positions, drone_radius, open_):
    """bool [P]: some agent j has norm(agent - position) < r_j + drone_radius, for the positions with open_[p].  numpy's norm is
    called only for the pairs whose plainly computed distance is within 1e-6 of the radius sum or below it: the two ways of
    computing a distance of some hundred px differ by a few units in the last place, 1e-13 at most."""
    dx = agents[A_PX][None, :] - positions[:, :1]
    dy = agents[A_PY][None, :] - positions[:, 1:]
    rr = agents[A_R] + drone_radius
    near = np.sqrt(dx * dx + dy * dy) < rr[None, :] + 1e-6
    out = np.zeros(len(positions), dtype=bool)
    for p, j in zip(*np.nonzero(near & open_[:, None])):
        if not out[p] and norm(np.array([agents[A_PX, j], agents[A_PY, j]]) - positions[p]) < agents[A_R, j] + drone_radius:
            out[p] = True
    return out


def fit_world(agents, positions, drone_radius, map_size, scale, dt, checks):
    """agents [6, N], positions [P, 2] -> dict of first [P] int32 (the index of the first check in which an agent touches the
    drone standing there, -1: none) and agents_end [6, N] (after checks + 1 updates): one update, then `checks` times (test every
    position, update)"""
    agents, positions = np.array(agents, dtype=np.float64), np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    first = np.full(len(positions), -1, dtype=np.int32)
    agents = agents_update(agents, map_size[0], map_size[1], scale, dt)
    for k in range(checks):
        first[hits(agents, positions, drone_radius, first < 0)] = k
        agents = agents_update(agents, map_size[0], map_size[1], scale, dt)
    return dict(first=first, agents_end=agents)


def fit_times(first, shape, T=12):
    """survive_times [X, Y] of the first hits: T where never hit, else the time of the check, then - 0.1 clamped at 0"""
    ts = np.arange(0, T, 0.1)
    survive = np.ones(shape) * T
    for p, k in enumerate(np.asarray(first).tolist()):
        if k >= 0:
            survive[p // shape[1], p % shape[1]] = min(ts[k], survive[p // shape[1], p % shape[1]])
    survive = survive - 0.1
    survive[survive < 0] = 0
    return survive
