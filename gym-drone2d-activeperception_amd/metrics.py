"""Difficulty metrics of the reference's script/difficulty_calculator/ on the device.

vo_calculator.py builds, for each seeded world and each of 16 x 16 drone positions, the velocity-obstacle cone of every agent and
asks for 63 x 10 candidate velocities whether any cone contains them; the fraction of free candidates is the position's rate, the
mean over the positions the world's metric (vo.csv).  Here the worlds of a batch, their positions and the candidates are three
launches of include/d2d_metrics.h (geometry, cones, count) with one host step between the first two: the cone's half angle
asin((rA + rB) / dist) goes through the host's libm over the flat array, because the device has no bit-exact asin yet.

    rates = vo_feasibility_batch(indices)          # [len(indices), 256]: per-position rates, 0 where the position is in collision
    metric = vo_feasibility(index)                 # np.mean(rates), as env_metrics(index) returns it
    table = vo_table()                             # the 20 x 27 nested list behind vo.csv
    table = density_table()                        # ... and behind density.csv (density_calculator.py, host arithmetic)
"""
import math
import time

import numpy as np
import torch

from . import _abi as A
from .params import Params
from .sweeps import _table_order
from .vec_env import build_worlds, build_worlds_device_of

VO_SCRIPT = 'script/difficulty_calculator/vo_calculator.py'
R_A = 5.0                                      # vo_calculator.py:57


def _params(index):
    """vo_calculator.py:38-48 / density_calculator.py:14-24.  drone_radius=0 changes the rejection sampling of the world: these are
    not the survivability sweep's worlds."""
    p = Params(agent_number=index['agent_number'], agent_radius=index['agent_size'], agent_max_speed=index['agent_speed'],
               map_id=index['map_id'], gaze_method='NoControl', planner='NoMove', drone_radius=0, debug=True,
               static_map='maps/empty_map.npy')
    p.render = False
    return p


def vo_positions(params, position_step=30):
    """x_range / y_range of vo_calculator.py:60-61."""
    lo = params.map_scale + params.drone_radius
    xs = list(range(lo, params.map_size[0] - params.map_scale - params.drone_radius, position_step))
    ys = list(range(lo, params.map_size[1] - params.map_scale - params.drone_radius, position_step))
    return xs, ys


def vo_candidates(v_min=20, v_max=60):
    """The candidate velocities of vo_calculator.py:101-103 in its loop order, float64 [630, 2], by the script's own expressions
    (np.arange, math.cos / math.sin, the products as numpy scalars)."""
    out = []
    for theta in np.arange(0, 2 * 3.14, 0.1):
        for rad in np.arange(v_min, v_max, (v_max - v_min) / 10.0):
            out.append([rad * math.cos(theta), rad * math.sin(theta)])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def _backend_of(backend, device):
    if backend is None:
        from ._lib import HipBackend
        backend = HipBackend(device)
    if not getattr(backend, 'supports_vo_metric', False):
        raise NotImplementedError(f'{getattr(backend, "name", type(backend).__name__)} has no velocity-obstacle metric '
                                  f'(include/d2d_metrics.h): run the reference\'s {VO_SCRIPT}')
    return backend


def host_asin(arg):
    """half = asin(arg) over the flat array through libm (math.asin, never np.arcsin: numpy may dispatch a vectorised routine of
    its own); 0 where arg > 1 -- those pairs belong to positions in collision, which the reference never evaluates."""
    flat = arg.reshape(-1).tolist()
    asin = math.asin
    return np.array([0.0 if v > 1.0 else asin(v) for v in flat], dtype=np.float64).reshape(arg.shape)


def vo_counts(agents, positions, cand, rA=R_A, backend=None, return_parts=False, timings=None):
    """The three launches plus the host asin.  agents [B, 6, N] (the state's layout), positions [P, 2], cand [C, 2]: float64 tensors
    on the backend's device.  Returns count [B, P] int32 (the suitable candidates; -1: the position is inside an agent's disc); with
    `return_parts` also a dict of arg, theta_ba, half [B, P, N], collided [B, P] and cone [B, P, N, 2].  `timings`: a dict that
    receives geometry_s, asin_s (D2H, asin, H2D), cones_s, count_s, each synchronised on both sides."""
    backend = _backend_of(backend, agents.device)
    dev = agents.device
    agents = agents.contiguous()
    positions = positions.to(torch.float64).contiguous()
    cand = cand.to(torch.float64).contiguous()
    if agents.dim() != 3 or agents.shape[1] != A.AF or positions.dim() != 2 or positions.shape[1] != 2 or cand.dim() != 2 or cand.shape[1] != 2:
        raise ValueError('vo_counts: agents [B, 6, N], positions [P, 2], cand [C, 2]')
    B, _, N = agents.shape
    P = positions.shape[0]
    arg = torch.empty((B, P, N), dtype=torch.float64, device=dev)
    theta_ba = torch.empty((B, P, N), dtype=torch.float64, device=dev)
    collided = torch.empty((B, P), dtype=torch.uint8, device=dev)
    cone = torch.empty((B, P, N, 2), dtype=torch.float64, device=dev)
    count = torch.empty((B, P), dtype=torch.int32, device=dev)

    def mark():
        if timings is not None:
            backend.sync()
        return time.perf_counter()
    t0 = mark()
    backend.vo_geometry(agents, positions, rA, arg, theta_ba, collided)
    t1 = mark()
    half = torch.from_numpy(host_asin(arg.cpu().numpy())).to(dev)
    t2 = mark()
    backend.vo_cones(theta_ba, half, collided, cone)
    t3 = mark()
    backend.vo_count(agents, cand, cone, collided, count)
    t4 = mark()
    if timings is not None:
        timings.update(geometry_s=t1 - t0, asin_s=t2 - t1, cones_s=t3 - t2, count_s=t4 - t3)
    if return_parts:
        return count, dict(arg=arg, theta_ba=theta_ba, half=half, collided=collided, cone=cone)
    return count


def vo_feasibility_batch(indices, position_step=30, device='cuda:0', backend=None, worlds=None, timings=None):
    """Per-position rates of several settings that share agent_number (same N), one chain of launches: float64
    [len(indices), P], count / C, 0 where the position is in collision (vo_calculator.py:95-97, :116), positions x-outermost.
    `worlds`: None (built here on the host, with drone_radius=0), a list of host worlds of `indices` built with _params(index), or
    'device' (built by the device, vec_env.build_worlds_device_of).
    `timings`: a dict that collects, per call, build_s, geometry_s, asin_s, cones_s, count_s and post_s (each synchronised on both
    sides) under 'batches', and their totals."""
    backend = _backend_of(backend, device)
    t_build = time.perf_counter()
    plist = [_params(ix) for ix in indices]
    xs, ys = vo_positions(plist[0], position_step)
    pos = np.array([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)
    cand = vo_candidates()
    dev = torch.device(backend.device)
    if isinstance(worlds, str):
        if worlds != 'device':
            raise ValueError(f"worlds {worlds!r}: a list of host worlds or 'device'")
        agents = build_worlds_device_of(plist, backend=backend).state.t['agents']
    else:
        seeded = worlds if worlds is not None else [build_worlds(p, 1)[0] for p in plist]
        if len(seeded) != len(plist):
            raise ValueError(f'vo_feasibility_batch: {len(seeded)} worlds for {len(plist)} settings')
        agents = torch.from_numpy(np.stack([np.asarray(w['agents'], dtype=np.float64) for w in seeded])).to(dev)
    if timings is not None:
        backend.sync()
    rec = {} if timings is not None else None
    t_dev = time.perf_counter()
    count = vo_counts(agents, torch.from_numpy(pos).to(dev), torch.from_numpy(cand).to(dev), R_A, backend, timings=rec)
    t_post = time.perf_counter()
    cnt = count.cpu().numpy()
    C = len(cand)
    rates = np.array([[0.0 if c < 0 else c / C for c in row] for row in cnt.tolist()], dtype=np.float64).reshape(cnt.shape)
    if timings is not None:
        rec.update(N=int(agents.shape[2]), worlds=len(plist), positions=len(pos), candidates=C, build_s=t_dev - t_build,
                   post_s=time.perf_counter() - t_post)
        timings.setdefault('batches', []).append(rec)
        for k in ('build_s', 'geometry_s', 'asin_s', 'cones_s', 'count_s', 'post_s', 'worlds'):
            timings[k] = timings.get(k, 0) + rec[k]
    return rates


def vo_feasibility(index, position_step=30, device='cuda:0', backend=None, worlds=None):
    """Drop-in for env_metrics(index) of vo_calculator.py:36-120: np.mean of the per-position rates."""
    return np.mean(vo_feasibility_batch([index], position_step, device, backend, worlds)[0])


def _by_agent_number(order, agent_numbers, fn):
    result = [None] * len(order)
    for n in dict.fromkeys(agent_numbers):       # one batch per agent count (a batch shares N)
        sel = [i for i, ix in enumerate(order) if ix['agent_number'] == n]
        for i, g in zip(sel, fn(sel)):
            result[i] = g
    return result


def vo_table(map_ids=range(20), agent_numbers=(10, 20, 30), agent_sizes=(5, 10, 15), agent_speeds=(20, 40, 60), position_step=30,
             device='cuda:0', backend=None, worlds=None, timings=None):
    """The nested list the reference writes to vo.csv (vo_calculator.py:122-136), in its loop order: one row per map_id, each with
    product(agent_num, agent_size, agent_vel) metrics.  `worlds`: None, 'device', or one host world per setting in that order."""
    map_ids = list(map_ids)
    order = _table_order(map_ids, agent_numbers, agent_sizes, agent_speeds)
    if worlds is not None and not isinstance(worlds, str) and len(worlds) != len(order):
        raise ValueError(f'vo_table: {len(worlds)} worlds for {len(order)} settings')

    def batch(sel):
        w = worlds if worlds is None or isinstance(worlds, str) else [worlds[i] for i in sel]
        return [np.mean(r) for r in vo_feasibility_batch([order[i] for i in sel], position_step, device, backend, w, timings)]
    flat = _by_agent_number(order, agent_numbers, batch)
    per_map = len(order) // max(len(map_ids), 1)
    return [flat[m * per_map:(m + 1) * per_map] for m in range(len(map_ids))]


def density(index, world=None):
    """Drop-in for env_metrics(index) of density_calculator.py:13-31: the Python-float sum of 3.14 * r ** 2 in agent order over
    map_size[0] * map_size[1], on the host.  The script builds its world with the reference's `gym-metric-v1` env, whose
    construction places the same random agents as `drone_v2` for these parameters: it differs only for static-map cells (radius
    1.414 * 5, other velocities; the script's map is empty) and for agent_radius == -1 (no (5, 15) range there)."""
    p = _params(index)
    if p.agent_radius == -1:
        raise NotImplementedError('density: gym-metric-v1 draws other radii than drone_v2 for agent_radius == -1; '
                                  'run the reference\'s script/difficulty_calculator/density_calculator.py')
    w = world if world is not None else build_worlds(p, 1)[0]
    obs_area = 0
    for r in np.asarray(w['agents'])[A.A_R].tolist():
        obs_area += 3.14 * r ** 2
    return obs_area / (p.map_size[0] * p.map_size[1])


def density_table(map_ids=range(20), agent_numbers=(10, 20, 30), agent_sizes=(5, 10, 15), agent_speeds=(20, 40, 60), worlds=None):
    """The nested list behind density.csv (density_calculator.py:33-51), in the same order as vo_table."""
    map_ids = list(map_ids)
    order = _table_order(map_ids, agent_numbers, agent_sizes, agent_speeds)
    if worlds is not None and len(worlds) != len(order):
        raise ValueError(f'density_table: {len(worlds)} worlds for {len(order)} settings')
    flat = [density(ix, None if worlds is None else worlds[i]) for i, ix in enumerate(order)]
    per_map = len(order) // max(len(map_ids), 1)
    return [flat[m * per_map:(m + 1) * per_map] for m in range(len(map_ids))]
