"""Shared inputs of the traversability / survival-fit tests: the recorded fixture, hand-made grids and agent worlds, and the Python
model's results (computed once per process and argument set)."""
import functools
import json
import os

import numpy as np

import drone2d_amd as pkg
from drone2d_amd import host_init, metrics, sweeps

import difficulty_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'difficulty_tables.npz')
KEYS = ('trav_agents', 'gt', 'distances', 'values', 'traversibility', 'trav_ref_seconds', 'fit_agents', 'survive_times', 'fit',
        'fit_agents_end', 'fit_ref_seconds')
AXIS_STARTS = [(x, y) for x in metrics.TRAV_AXIS for y in metrics.TRAV_AXIS]
MAP = dict(map_size=(500, 500), scale=10, dt=0.1, drone_radius=10)          # the fit worlds' constants (Params' defaults)
CHECKS = 120


@functools.lru_cache(maxsize=None)
def fixture():
    """[(index, dict of KEYS)] of the five settings"""
    z = np.load(GOLD)
    return [(json.loads(str(z[f's{i}_index'])), {k: z[f's{i}_{k}'] for k in KEYS}) for i in range(int(z['n']))]


def world_of(params):
    return host_init.init_world(pkg.with_defaults(params))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def positions_of(params, step=60):
    xs, ys = sweeps.start_cells(params, step)
    return np.array([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def fixture_trav_model(i):
    return M.trav_world(fixture()[i][1]['gt'], AXIS_STARTS)


@functools.lru_cache(maxsize=None)
def fixture_fit_model(i, checks=CHECKS):
    index, rec = fixture()[i]
    p = sweeps._params(index)
    return M.fit_world(rec['fit_agents'], positions_of(p), p.drone_radius, p.map_size, p.map_scale, p.dt, checks)


# ---- hand-made grids

@functools.lru_cache(maxsize=None)
def small_grid():
    """7 x 5 (W != H), open but for one cell of each other value: 0 (unexplored), 1 (occupied), 3 -- each stops a ray"""
    g = np.full((7, 5), 2, dtype=np.uint8)
    g[1, 3], g[4, 1], g[5, 3] = 0, 1, 3
    return g


# corners, edges (walks of 0 steps, diagonals that end at the border), the middle, and the three cells that are not open
SMALL_STARTS = [(0, 0), (6, 4), (0, 4), (6, 0), (0, 2), (3, 0), (6, 2), (3, 4), (3, 2), (2, 2), (1, 3), (4, 1), (5, 3)]


@functools.lru_cache(maxsize=None)
def random_grid(W, H, seed, wall=0.03):
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(W, H) < wall, rng.choice([0, 1, 3], (W, H)), 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def random_starts(W, H, S, seed):
    rng = np.random.RandomState(seed)
    return [(int(rng.randint(W)), int(rng.randint(H))) for _ in range(S)]


@functools.lru_cache(maxsize=None)
def grid_model(name, *args):
    grid, starts = GRIDS[name](*args)
    return M.trav_steps(grid, starts)


GRIDS = {
    'small': lambda: (small_grid(), SMALL_STARTS),
    'random': lambda W, H, S, seed: (random_grid(W, H, seed), random_starts(W, H, S, seed + 1)),
}


# ---- hand-made agents

@functools.lru_cache(maxsize=None)
def adversarial_agents(touching=False):
    """One 500 x 500 world of N = 70 agents [6, N]; its first 1, 24, 64, 65 agents are worlds of their own.
      0   at rest at (80, 97), r = 7: at distance r + drone_radius from the position (80, 80) exactly, for ever -- not a hit; alone
          (N = 1) it is a world that is never hit.  `touching`: 0.001 px nearer, a hit at check 0
      1-4 aimed at the left, right, top and bottom wall, two steps away from it
      5   in the corner: its first step bounces on both axes
      6   of speed 4: turned by the stuck-agent rule in every step
      7, 8  of speed 5 exactly, (3, 4) and (5, 0): the rule's boundary
      9   of speed 5.000001
    the rest random with speeds of 0 to 60, clear of nothing: they cross the positions at their own times."""
    rng = np.random.RandomState(33)
    N = 70
    x, y = rng.uniform(30, 470, N), rng.uniform(30, 470, N)
    speed, ang = rng.uniform(0, 60, N), rng.uniform(0, 2 * np.pi, N)
    vx, vy, r = speed * np.cos(ang), speed * np.sin(ang), rng.uniform(4, 16, N)
    fixed = {0: (80.0, 96.999 if touching else 97.0, 0.0, 0.0, 7.0), 1: (25.0, 250.0, -40.0, 3.0, 8.0), 2: (474.0, 200.0, 40.0, -2.0, 9.0),
             3: (300.0, 24.0, 1.0, -40.0, 7.5), 4: (310.0, 473.0, -1.0, 40.0, 10.0), 5: (19.0, 19.5, -30.0, -30.0, 8.0),
             6: (150.0, 150.0, 4.0, 0.0, 6.0), 7: (200.0, 300.0, 3.0, 4.0, 6.0), 8: (350.0, 120.0, 5.0, 0.0, 6.0),
             9: (400.0, 400.0, 5.000001, 0.0, 6.0)}
    for k, v in fixed.items():
        x[k], y[k], vx[k], vy[k], r[k] = v
    return np.stack([x, y, vx, vy, r, r ** 2])


@functools.lru_cache(maxsize=None)
def many_agents(N):
    """N <= 280 agents: the adversarial world four times over, each copy moved and turned a little (worlds of three and four tiles
    of 64 agents)"""
    ag = adversarial_agents()
    parts = []
    for k in range(4):
        c = ag.copy()
        c[0] = 30 + (c[0] - 30 + 37.25 * k) % 440
        c[1] = 30 + (c[1] - 30 + 61.5 * k) % 440
        c[2], c[3] = c[2] - 0.75 * k * c[3], c[3] + 0.5 * k * c[2]
        parts.append(c)
    return np.concatenate(parts, axis=1)[:, :N].copy()


@functools.lru_cache(maxsize=None)
def many_agents_model(N, checks=40):
    ag = many_agents(N)
    return ag, M.fit_world(ag, fit_positions(64), 10, MAP['map_size'], MAP['scale'], MAP['dt'], checks)


@functools.lru_cache(maxsize=None)
def adversarial_fit_model(N, P=64, checks=CHECKS, drone_radius=10, touching=False, roll=0):
    ag = np.roll(adversarial_agents(touching)[:, :N], roll, axis=1)
    return ag, M.fit_world(ag, fit_positions(P), drone_radius, MAP['map_size'], MAP['scale'], MAP['dt'], checks)


@functools.lru_cache(maxsize=None)
def fit_positions(P):
    """P = 1: (80, 80); 64: the script's 8 x 8; 65: and one between them"""
    pos = np.array([(x, y) for x in range(20, 480, 60) for y in range(20, 480, 60)], dtype=np.float64)
    if P == 1:
        return pos[9:10].copy()
    return pos if P == 64 else np.concatenate([pos, [[251.5, 247.25]]])
