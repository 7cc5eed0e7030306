"""Synthetic batches for the Jerk_Primitive planner's tests (test_jerk_host_build.py, test_gpu_jerk.py): arrays in the layouts of
include/d2d_jerk.h, the scenes tests/jerk_model.py reads, and the model's answers, computed once per batch and shared.

Env e of a batch is of kind e % len(KINDS):
  open       random drone, goal, velocity and acceleration; random walls; the env's trackers move
  axis       goal straight along an axis or a diagonal (phi_h a multiple of 45: on a heading, 35 tied pairs); 1 to 3 of the best
             headings are blocked by point-sized trackers (N >= 3) so that a tied pair decides
  wall       goal along an axis, a wall across the whole map ahead of the drone: the first free headings are a tied pair
  on_pf      goal exactly on the end point of the best heading: norm(l) = 0, NaN samples for that heading, then a tied pair
  border     drone next to one of the four borders
  blocked    every cell of the map occupied: no plan
  archived   open, with trackers that were active at the step before and are not any more (their radius goes back to agent_radius)
"""
import functools

import numpy as np

import jerk_model as M

KINDS = ('open', 'axis', 'wall', 'on_pf', 'border', 'blocked', 'archived')
KF, DF = 20, 8
AGENT_RADIUS = 10.0
DRONE_RADIUS = 10.0
SCALE = 10
DT = 0.1

# (B, N, v_max, W, H, tile): the device test's batches; the host build runs the same ones with fewer envs
BATCHES = [(257, 0, 40, 50, 50, 0), (257, 3, 20, 50, 50, 0), (257, 70, 40, 37, 45, 16), (257, 3, 7, 37, 45, 16), (257, 3, 72, 50, 50, 0)]


def tile_grid(g, tile):
    """[W, H] -> the bytes of one env's grid in 16 x 16 tiles (include/d2d.h, d2d_cfg.grid_tile)"""
    W, H = g.shape
    Wt, Ht = (W + tile - 1) // tile, (H + tile - 1) // tile
    pad = np.zeros((Wt * tile, Ht * tile), dtype=g.dtype)
    pad[:W, :H] = g
    return pad.reshape(Wt, tile, Ht, tile).transpose(0, 2, 1, 3).reshape(-1).copy()


def scene_of(b, e):
    act = b['active'][e].astype(bool)
    return dict(drone=tuple(b['drone'][e][[0, 1, 3, 4, 5, 6]]), target=tuple(b['target'][e]), dmap=b['dmap'][e],
                trackers=[(b['kf'][e, k, :4], b['radius_after'][e, k]) for k in range(b['N']) if act[k]],
                scale=SCALE, map_size=(b['W'] * SCALE, b['H'] * SCALE), drone_radius=DRONE_RADIUS, var_cam=b['var_cam'],
                v_max=b['v_max'], dt=DT)


@functools.lru_cache(maxsize=None)
def batch(B, N, v_max, W, H, tile, seed=0):
    rng = np.random.RandomState(1000 + 7 * N + v_max + W + seed)
    W_px, H_px = W * SCALE, H * SCALE
    drone = np.zeros((B, DF))
    target = np.zeros((B, 2))
    active = np.zeros((B, max(N, 1)), dtype=np.uint8)[:, :N]
    kf = np.zeros((B, N, KF))
    dmap = np.full((B, W, H), 2, dtype=np.uint8)
    radius0 = np.full((B, N), AGENT_RADIUS) + rng.randint(-2, 3, (B, N))
    prev = np.zeros((B, N), dtype=np.uint8)
    kinds = [KINDS[e % len(KINDS)] for e in range(B)]
    b = dict(B=B, N=N, v_max=v_max, W=W, H=H, tile=tile, var_cam=0.0 if seed % 2 == 0 else 2.0, kinds=kinds)
    for e, kind in enumerate(kinds):
        g = dmap[e]
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1
        x, y = rng.randint(60, W_px - 60), rng.randint(60, H_px - 60)
        vel, acc = rng.uniform(-v_max / 2, v_max / 2, 2), rng.uniform(-10, 10, 2)
        goal = np.array([rng.randint(30, W_px - 30), rng.randint(30, H_px - 30)], dtype=np.float64)
        if kind in ('open', 'archived'):
            for _ in range(3):
                i, j = rng.randint(1, W - 3), rng.randint(1, H - 3)
                g[i:i + 2, j:j + 2] = 1
            g[rng.randint(1, W - 1), rng.randint(1, H - 1)] = 3      # a DYNAMIC cell: not a wall for the planner
            g[rng.randint(1, W - 1), rng.randint(1, H - 1)] = 0
        if kind in ('axis', 'wall', 'on_pf'):
            x, y = W_px // 2 + rng.randint(-20, 20), H_px // 2 + rng.randint(-20, 20)
            dirs = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]
            dx, dy = dirs[(e // len(KINDS)) % (4 if kind != 'axis' else 8)]
            reach = 30 if kind == 'on_pf' else rng.randint(40, 120)
            goal = np.array([x + dx * reach, y + dy * reach], dtype=np.float64)
            if kind == 'on_pf':
                vel, acc = np.zeros(2), np.zeros(2)
            if kind == 'wall':                               # occupied from 30 px ahead of the drone to the border
                vel = acc = np.zeros(2)
                if dx:
                    cells = range((x + 30) // SCALE, W) if dx > 0 else range(0, (x - 30) // SCALE + 1)
                    g[list(cells), :] = 1
                else:
                    cells = range((y + 30) // SCALE, H) if dy > 0 else range(0, (y - 30) // SCALE + 1)
                    g[:, list(cells)] = 1
        if kind == 'border':
            side = (e // len(KINDS)) % 4
            x, y = [(12, y), (W_px - 13, y), (x, 12), (x, H_px - 13)][side]
        if kind == 'blocked':
            g[:, :] = 1
        drone[e] = [x, y, rng.uniform(0, 360), vel[0], vel[1], acc[0], acc[1], 0.0]
        target[e] = goal
        for k in range(N):                                   # moving trackers somewhere on the map, about a third of them active
            kf[e, k, :4] = [rng.uniform(20, W_px - 20), rng.uniform(20, H_px - 20), rng.uniform(-20, 20), rng.uniform(-20, 20)]
            kf[e, k, 4:] = rng.uniform(0, 1, 16)
            active[e, k] = rng.rand() < 0.34 and kind in ('open', 'archived', 'border')
            prev[e, k] = active[e, k]
        if kind == 'archived' and N:
            gone = rng.choice(N, max(1, N // 3), replace=False)
            prev[e, gone], active[e, gone] = 1, 0
        if kind == 'axis' and N >= 3:
            # point-sized stationary trackers (limit 0.5 px) on the last sample of the best `depth` ranks' headings: those and only
            # those are blocked -- neighbouring headings end 2.6 px apart
            sc = dict(drone=(x, y, vel[0], vel[1], acc[0], acc[1]), target=tuple(goal), v_max=v_max, dt=DT)
            order = np.argsort(M.costs(M.goal_direction(sc)), kind='stable')
            depth = 1 + (e // (8 * len(KINDS))) % 3
            block = [order[0]] if depth == 1 else [order[0], order[1], order[2]] if depth == 2 else [order[0], order[1]]
            for k, i in enumerate(block[:N]):
                p = M.primitive(sc, 5.0 * i)[0]
                kf[e, k, :4] = [p[-1, 0], p[-1, 1], 0.0, 0.0]
                radius0[e, k] = 0.5 - DRONE_RADIUS - 5 - b['var_cam']
                active[e, k] = prev[e, k] = 1
    radius_after = radius0.copy()
    prev_after = prev.copy()
    for e in range(B):
        M.step_trackers(radius_after[e], prev_after[e], active[e], AGENT_RADIUS)
    b.update(drone=drone, target=target, active=np.ascontiguousarray(active), kf=kf, dmap=dmap, radius0=radius0, prev=prev,
             radius_after=radius_after, prev_after=prev_after,
             dmap_bytes=np.stack([tile_grid(g, tile) if tile else g.reshape(-1) for g in dmap]))
    return b


@functools.lru_cache(maxsize=None)
def answers(B, N, v_max, W, H, tile, seed=0):
    """the model's decision for every env of batch(...): dict of arrays plan_ok [B], choice [B], wp [B, 6], tie [B], tested [B],
    unknown [B] (the tie table of this host does not describe the env's costs although they hold a tie)"""
    from drone2d_amd import jerk_plugin as JP
    b = batch(B, N, v_max, W, H, tile, seed)
    perm, eq = tie()
    out = dict(plan_ok=np.zeros(B, np.uint8), choice=np.zeros(B, np.int32), wp=np.zeros((B, 6)), tie=np.zeros(B, bool),
               tested=np.zeros(B, np.int32), unknown=np.zeros(B, bool))
    for e in range(B):
        r = M.plan(scene_of(b, e))
        for k in ('plan_ok', 'choice', 'wp', 'tie', 'tested'):
            out[k][e] = r[k]
        pat = JP.pattern_of(r['phi_h'])
        srt = np.sort(r['cost'])
        out['unknown'][e] = not JP.table_fits(perm[pat], eq[pat], r['cost']) and bool((srt[1:] == srt[:-1]).any())
    return out


@functools.lru_cache(maxsize=None)
def tie():
    from drone2d_amd import jerk_plugin as JP
    return JP.tie_table()


@functools.lru_cache(maxsize=None)
def tables(v_max):
    from drone2d_amd import jerk_plugin as JP
    return JP.primitive_tables(v_max, DT)


def call_of(b, ptr, arrays):
    """the d2d_jerk_call of batch `b`; ptr(x) is the address of array x where the library will read it.  `arrays`: name -> array for
    every pointer of the call"""
    from drone2d_amd import _abi as A
    c = A.JerkCall()
    for k in A.JERK_CALL_POINTERS:
        setattr(c, k, ptr(arrays[k]) if arrays[k] is not None else None)
    c.B, c.N, c.S, c.W, c.H, c.grid_tile = b['B'], b['N'], arrays['tt_tab'].shape[1], b['W'], b['H'], b['tile']
    c.scale, c.W_px, c.H_px = SCALE, b['W'] * SCALE, b['H'] * SCALE
    c.drone_radius, c.agent_radius, c.var_cam, c.half_v_max = DRONE_RADIUS, AGENT_RADIUS, b['var_cam'], 0.5 * b['v_max']
    return c


def host_arrays(b):
    """fresh numpy inputs and outputs of one call on batch `b` (outputs poisoned)"""
    th, tt, S = tables(b['v_max'])
    perm, eq = tie()
    B, N = b['B'], b['N']
    some = lambda a: np.ascontiguousarray(a) if a.size else None   # noqa: E731
    return dict(drone=b['drone'].copy(), target=b['target'].copy(), active=some(b['active'].copy()), kf=some(b['kf'].copy()),
                dmap=b['dmap_bytes'].copy(), trk_radius=some(b['radius0'].copy()), trk_prev=some(b['prev'].copy()),
                th_tab=th.copy(), tt_tab=tt.copy(), tie_perm=perm.copy(), tie_eq=eq.copy(),
                plan_ok=np.full(B, 7, np.uint8), wp_valid=np.full(B, 7, np.uint8), wp=np.full((B, 6), np.nan),
                choice=np.full(B, -9, np.int32), stat=np.full(B, -9, np.int32))
