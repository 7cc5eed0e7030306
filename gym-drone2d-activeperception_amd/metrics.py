"""Difficulty metrics of the reference's script/difficulty_calculator/ on the device.

vo_calculator.py builds, for each seeded world and each of 16 x 16 drone positions, the velocity-obstacle cone of every agent and
asks for 63 x 10 candidate velocities whether any cone contains them; the fraction of free candidates is the position's rate, the
mean over the positions the world's metric (vo.csv).  Here the worlds of a batch, their positions and the candidates are three
launches of include/d2d_metrics.h (geometry, cones, count) with nothing between them: the cone's half angle asin((rA + rB) / dist)
is taken inside the second launch by the device's restatement of libm's asin (asin='device', the default; device_asin() is that
function alone).  asin='host' is the earlier path, with the same bits: the half angle goes through the host's libm over the flat
array between the first two launches (host_asin).

    rates = vo_feasibility_batch(indices)          # [len(indices), 256]: per-position rates, 0 where the position is in collision
    metric = vo_feasibility(index)                 # np.mean(rates), as env_metrics(index) returns it
    table = vo_table()                             # the 20 x 27 nested list behind vo.csv
    table = density_table()                        # ... and behind density.csv (density_calculator.py, host arithmetic)

traversibility_calculator.py walks the ground-truth grid of each seeded world from 9 x 9 start cells in eight directions
(traversibility.csv); survivability_calculator.py moves the agents of each world for 12 s and records when a drone standing at each of
8 x 8 positions is first hit (metrics_fit.csv, the table script/fit.py fits the difficulty model to).  Each is one launch per batch
(d2d_trav_steps, d2d_fit_first_hit) that returns integers -- steps walked, the index of the first check that hit -- and the host
turns them into the reference's floats with the reference's own expressions.

    values = traversibility_batch(indices)         # [len(indices), 81]: per-start mean distance, 0 where the start is occupied
    metric = traversibility(index)                 # their running sum / 81, as env_metrics(index) returns it
    table = traversibility_table()                 # the 20 x 27 nested list behind traversibility.csv
    times = survival_fit_batch(indices)            # [len(indices), 8, 8]: survive_times after the - 0.1 and the clamp
    metric = survival_fit(index)                   # np.mean(times), as env_metrics(index) returns it
    table = survival_fit_table()                   # the 1 x 800 nested list behind metrics_fit.csv
"""
import math
import time

import numpy as np
import torch

from . import _abi as A
from ._lib import backend_for
from .params import Params
from . import sweeps
from .sweeps import _host_worlds, _on_device, _per_agent_count, _record, _table_order
from .vec_env import build_worlds, build_worlds_device_of

VO_SCRIPT = 'script/difficulty_calculator/vo_calculator.py'
TRAV_SCRIPT = 'script/difficulty_calculator/traversibility_calculator.py'
FIT_SCRIPT = 'script/difficulty_calculator/survivability_calculator.py'
TRAV_AXIS = (5, 10, 15, 20, 25, 30, 35, 40, 45)     # traversibility_calculator.py:29
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


def _backend_of(backend, device, script):
    """The backend of a metric of `script` (backend_for): one with the velocity-obstacle kernels for VO_SCRIPT, with the
    traversability / survival-fit kernels for the other two."""
    flag, what = ('supports_vo_metric', 'velocity-obstacle') if script == VO_SCRIPT else \
        ('supports_difficulty_tables', 'traversability / survival-fit')
    return backend_for(backend, device, flag, f'has no {what} metric (include/d2d_metrics.h): run the reference\'s {script}')


def _seeded_worlds(who, plist, worlds, backend, fields):
    """The tensors `fields` ('agents', 'gt') of the seeded worlds of `plist` on the backend's device: built here on the host
    (worlds=None), taken from a list of host worlds, or built by the device (worlds='device'; the grid in the reference's [W][H]
    indexing whatever layout the device keeps)."""
    dev = torch.device(backend.device)
    if _on_device(worlds):
        state = build_worlds_device_of(plist, backend=backend).state
        return [state.logical(f).contiguous() for f in fields]
    seeded = _host_worlds(who, plist, worlds)
    dtype = dict(agents=np.float64, gt=np.uint8)
    return [torch.from_numpy(np.stack([np.asarray(w[f], dtype=dtype[f]) for w in seeded])).to(dev) for f in fields]


def host_asin(arg):
    """half = asin(arg) over the flat array through libm (math.asin, never np.arcsin: numpy may dispatch a vectorised routine of
    its own); 0 where arg > 1 -- those pairs belong to positions in collision, which the reference never evaluates."""
    flat = arg.reshape(-1).tolist()
    asin = math.asin
    return np.array([0.0 if v > 1.0 else asin(v) for v in flat], dtype=np.float64).reshape(arg.shape)


ASIN_PATHS = ('device', 'host')


def _asin_path(who, asin):
    if asin not in ASIN_PATHS:
        raise ValueError(f'{who}: asin={asin!r}: \'device\' (the half angle inside the cones launch) or \'host\' (libm between the launches)')
    return asin


def device_asin(x, backend=None):
    """libm's asin of a float64 tensor on the backend's device, bit for bit (d2d_asin_array): what math.asin returns for every
    element of [-1, 1], NaN for NaN and where math.asin raises (|x| > 1).  Returns a new tensor of x's shape."""
    backend = _backend_of(backend, x.device, VO_SCRIPT)
    if x.dtype != torch.float64:
        raise ValueError('device_asin: a float64 tensor')
    x = x.contiguous()
    out = torch.empty_like(x)
    if x.numel():                          # (an empty tensor has no storage: its pointer is NULL, which the library refuses)
        backend.asin_array(x, out)
    return out


def vo_counts(agents, positions, cand, rA=R_A, backend=None, return_parts=False, timings=None, asin='device'):
    """The three launches.  agents [B, 6, N] (the state's layout), positions [P, 2], cand [C, 2]: float64 tensors on the backend's
    device.  Returns count [B, P] int32 (the suitable candidates; -1: the position is inside an agent's disc); with `return_parts`
    also a dict of arg, theta_ba, half [B, P, N], collided [B, P] and cone [B, P, N, 2].  `asin`: 'device' takes the half angle
    inside the cones launch (d2d_vo_cones_arg; nothing crosses to the host), 'host' between the launches through the host's libm
    (host_asin, then d2d_vo_cones); the results are the same bits.  `timings`: a dict that receives geometry_s, asin_s (D2H, asin,
    H2D; 0.0 with asin='device', where cones_s covers the asin and the cones in their one launch), cones_s, count_s, each
    synchronised on both sides."""
    _asin_path('vo_counts', asin)
    backend = _backend_of(backend, agents.device, VO_SCRIPT)
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
    if asin == 'device':
        t2 = t1
        half = torch.empty((B, P, N), dtype=torch.float64, device=dev) if return_parts else None
        backend.vo_cones_arg(theta_ba, arg, collided, half, cone)
    else:
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


def vo_feasibility_batch(indices, position_step=30, device='cuda:0', backend=None, worlds=None, timings=None, asin='device'):
    """Per-position rates of several settings that share agent_number (same N), one chain of launches: float64
    [len(indices), P], count / C, 0 where the position is in collision (vo_calculator.py:95-97, :116), positions x-outermost.
    `worlds`: None (built here on the host, with drone_radius=0), a list of host worlds of `indices` built with _params(index), or
    'device' (built by the device, vec_env.build_worlds_device_of).  `asin`: as in vo_counts.
    `timings`: a dict that collects, per call, build_s, geometry_s, asin_s, cones_s, count_s and post_s (each synchronised on both
    sides) under 'batches', and their totals; asin_s is 0.0 with asin='device' (cones_s covers the fused launch)."""
    _asin_path('vo_feasibility_batch', asin)
    backend = _backend_of(backend, device, VO_SCRIPT)
    t_build = time.perf_counter()
    plist = [_params(ix) for ix in indices]
    xs, ys = vo_positions(plist[0], position_step)
    pos = np.array([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)
    cand = vo_candidates()
    agents, = _seeded_worlds('vo_feasibility_batch', plist, worlds, backend, ('agents',))
    dev = agents.device
    if timings is not None:
        backend.sync()
    rec = {} if timings is not None else None
    t_dev = time.perf_counter()
    count = vo_counts(agents, torch.from_numpy(pos).to(dev), torch.from_numpy(cand).to(dev), R_A, backend, timings=rec, asin=asin)
    t_post = time.perf_counter()
    cnt = count.cpu().numpy()
    C = len(cand)
    rates = np.array([[0.0 if c < 0 else c / C for c in row] for row in cnt.tolist()], dtype=np.float64).reshape(cnt.shape)
    if timings is not None:
        rec.update(N=int(agents.shape[2]), worlds=len(plist), positions=len(pos), candidates=C, build_s=t_dev - t_build,
                   post_s=time.perf_counter() - t_post)
        _record(timings, rec, ('build_s', 'geometry_s', 'asin_s', 'cones_s', 'count_s', 'post_s', 'worlds'))
    return rates


def vo_feasibility(index, position_step=30, device='cuda:0', backend=None, worlds=None, asin='device'):
    """Drop-in for env_metrics(index) of vo_calculator.py:36-120: np.mean of the per-position rates."""
    return np.mean(vo_feasibility_batch([index], position_step, device, backend, worlds, asin=asin)[0])


def _table(who, order, map_ids, agent_numbers, worlds, batch):
    """The nested list of a difficulty table: one batch(indices, their worlds) per agent count (sweeps._per_agent_count), its
    metrics put back in the order of `order` and cut into one row per map_id."""
    flat = _per_agent_count(who, order, agent_numbers, worlds, batch)
    per_map = len(order) // max(len(map_ids), 1)
    return [flat[m * per_map:(m + 1) * per_map] for m in range(len(map_ids))]


def vo_table(map_ids=range(20), agent_numbers=(10, 20, 30), agent_sizes=(5, 10, 15), agent_speeds=(20, 40, 60), position_step=30,
             device='cuda:0', backend=None, worlds=None, timings=None, asin='device'):
    """The nested list the reference writes to vo.csv (vo_calculator.py:122-136), in its loop order: one row per map_id, each with
    product(agent_num, agent_size, agent_vel) metrics.  `worlds`: None, 'device', or one host world per setting in that order.
    `asin`: as in vo_counts."""
    _asin_path('vo_table', asin)
    map_ids = list(map_ids)
    order = _table_order(map_ids, agent_numbers, agent_sizes, agent_speeds)

    kw = {} if asin == 'device' else dict(asin=asin)      # the default path through the batch function's earlier signature

    def batch(indices, w):
        return [np.mean(r) for r in vo_feasibility_batch(indices, position_step, device, backend, w, timings, **kw)]
    return _table('vo_table', order, map_ids, agent_numbers, worlds, batch)


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

    def batch(indices, w):
        return [density(ix, None if w is None else w[k]) for k, ix in enumerate(indices)]
    return _table('density_table', order, map_ids, agent_numbers, worlds, batch)


# ---- traversibility_calculator.py and survivability_calculator.py

def trav_steps(gt, starts, backend=None):
    """One launch of d2d_trav_steps.  gt [B, W, H] uint8 on the backend's device, in the reference's indexing; starts: S pairs
    (i, j) of host integers.  Returns steps [B, S, 8] int32 on the device: the steps walked towards N, NE, E, SE, S, SW, W, NW, or
    -1 in all eight where the start cell is not UNOCCUPIED.  A start outside the grid is refused here, before it is uploaded: the
    library cannot look into device memory before its launch."""
    backend = _backend_of(backend, gt.device, TRAV_SCRIPT)
    st = np.asarray(starts, dtype=np.int64).reshape(-1, 2)
    if gt.dim() != 3 or gt.dtype != torch.uint8 or len(st) < 1:
        raise ValueError('trav_steps: gt [B, W, H] uint8, starts [S, 2] with S >= 1')
    B, W, H = gt.shape
    if (st < 0).any() or (st[:, 0] >= W).any() or (st[:, 1] >= H).any():
        bad = st[(st < 0).any(axis=1) | (st[:, 0] >= W) | (st[:, 1] >= H)][0]
        raise ValueError(f'trav_steps: start ({int(bad[0])}, {int(bad[1])}) lies outside the {W} x {H} grid')
    steps = torch.empty((B, len(st), 8), dtype=torch.int32, device=gt.device)
    backend.trav_steps(gt.contiguous(), torch.from_numpy(st.astype(np.int32)).to(gt.device), steps)
    return steps


_DIAGONAL = [0]     # _DIAGONAL[k]: `distance` of traversibility.py:37-46 after k diagonal steps (0, then k times += math.sqrt(2))


def _diagonal(k):
    while len(_DIAGONAL) <= k:
        _DIAGONAL.append(_DIAGONAL[-1] + math.sqrt(2))
    return _DIAGONAL[k]


def trav_values(steps):
    """traversibility.py:32-51 from step counts [..., 8] (host integers): per start the np.mean of the eight distances -- the
    straight ones the int k, the diagonal ones the k-fold `distance += math.sqrt(2)` -- or 0 where the start is not UNOCCUPIED."""
    st = np.asarray(steps)
    out = []
    for row in st.reshape(-1, 8).tolist():
        out.append(0 if row[0] < 0 else np.mean([_diagonal(k) if d % 2 else k for d, k in enumerate(row)]))
    return np.array(out, dtype=np.float64).reshape(st.shape[:-1])


def trav_metric(values):
    """metric_env.py:288-293: the running sum of the per-start values in start order over their number"""
    travers_sum = 0
    vals = np.asarray(values, dtype=np.float64).tolist()
    for v in vals:
        travers_sum += v
    return travers_sum / len(vals)


def traversibility_batch(indices, axis_range=TRAV_AXIS, device='cuda:0', backend=None, worlds=None, timings=None):
    """Per-start traversability of several settings that share agent_number (same N, for the device's world construction), one
    launch: float64 [len(indices), len(axis_range) ** 2], starts in the order of product(axis_range, axis_range), 0 where the
    start cell is occupied.  The worlds are the VO metric's (_params: drone_radius=0), whose ground-truth grid at reset is the one
    the reference's gym-metric-v1 env builds for these parameters.  `worlds`: as in vo_feasibility_batch.
    `timings`: a dict that collects, per call, build_s, launch_s, d2h_s and post_s (each synchronised on both sides) under
    'batches', and their totals."""
    backend = _backend_of(backend, device, TRAV_SCRIPT)
    t0 = time.perf_counter()
    for ix in indices:
        if ix['agent_size'] == -1:
            raise NotImplementedError('traversibility: gym-metric-v1 draws other radii than drone_v2 for agent_radius == -1; '
                                      f'run the reference\'s {TRAV_SCRIPT}')
    plist = [_params(ix) for ix in indices]
    axis = list(axis_range)
    starts = [(x, y) for x in axis for y in axis]
    gt, = _seeded_worlds('traversibility_batch', plist, worlds, backend, ('gt',))
    if timings is not None:
        backend.sync()
    t1 = time.perf_counter()
    steps = trav_steps(gt, starts, backend)
    if timings is not None:
        backend.sync()
    t2 = time.perf_counter()
    host = steps.cpu().numpy()
    t3 = time.perf_counter()
    values = trav_values(host)
    if timings is not None:
        _record(timings, dict(worlds=len(plist), starts=len(starts), build_s=t1 - t0, launch_s=t2 - t1, d2h_s=t3 - t2,
                              post_s=time.perf_counter() - t3), ('worlds', 'build_s', 'launch_s', 'd2h_s', 'post_s'))
    return values


def traversibility(index, axis_range=TRAV_AXIS, device='cuda:0', backend=None, worlds=None):
    """Drop-in for env_metrics(index) of traversibility_calculator.py:13-32."""
    return trav_metric(traversibility_batch([index], axis_range, device, backend, worlds)[0])


def traversibility_table(map_ids=range(20), agent_numbers=(10, 20, 30), agent_sizes=(5, 10, 15), agent_speeds=(20, 40, 60),
                         axis_range=TRAV_AXIS, device='cuda:0', backend=None, worlds=None, timings=None):
    """The nested list the reference writes to traversibility.csv (traversibility_calculator.py:34-52), in its loop order: one row
    per map_id, each with product(agent_num, agent_size, agent_vel) metrics.  `worlds`: as in vo_table."""
    map_ids = list(map_ids)
    order = _table_order(map_ids, agent_numbers, agent_sizes, agent_speeds)

    def batch(indices, w):
        return [trav_metric(v) for v in traversibility_batch(indices, axis_range, device, backend, w, timings)]
    return _table('traversibility_table', order, map_ids, agent_numbers, worlds, batch)


def fit_first_hit(agents, positions, params, checks, backend=None, return_agents=False):
    """One launch of d2d_fit_first_hit.  agents [B, 6, N] (the state's layout) and positions [P, 2]: float64 tensors on the
    backend's device; params: map_size, map_scale, dt and drone_radius of the worlds.  Returns first [B, P] int32 (the index of the
    first of `checks` checks in which an agent touched the drone standing there, -1: none did); with `return_agents` also the agents
    after the checks + 1 updates."""
    backend = _backend_of(backend, agents.device, FIT_SCRIPT)
    agents = agents.contiguous()
    positions = positions.to(torch.float64).contiguous()
    if agents.dim() != 3 or agents.shape[1] != A.AF or agents.dtype != torch.float64 or positions.dim() != 2 or positions.shape[1] != 2:
        raise ValueError('fit_first_hit: agents [B, 6, N] float64, positions [P, 2]')
    first = torch.empty((agents.shape[0], positions.shape[0]), dtype=torch.int32, device=agents.device)
    out = torch.empty_like(agents) if return_agents else None
    backend.fit_first_hit(agents, positions, params.drone_radius, params.map_size[0], params.map_size[1], params.map_scale, params.dt,
                          checks, first, out)
    return (first, out) if return_agents else first


def fit_times(first, T=12):
    """survivability_calculator.py:30, :34, :40, :45-46 from the index of the first check that hit [...] (host integers, -1: none):
    np.ones(...) * T, min(t, .) with t = np.arange(0, T, 0.1)[first], then - 0.1 and the clamp at 0."""
    first = np.asarray(first)
    ts = np.arange(0, T, 0.1)
    survive_times = np.ones(first.shape) * T
    flat = survive_times.reshape(-1)
    for i, k in enumerate(first.reshape(-1).tolist()):
        if k >= 0:
            flat[i] = min(ts[k], flat[i])
    survive_times = survive_times - 0.1
    survive_times[survive_times < 0] = 0
    return survive_times


def survival_fit_batch(indices, position_step=60, T=12, device='cuda:0', backend=None, worlds=None, timings=None, return_agents=False):
    """survive_times of several settings that share agent_number (same N), one launch: float64 [len(indices), len(x_range),
    len(y_range)] after the - 0.1 and the clamp (survivability_calculator.py:45-46), positions x-outermost (sweeps.start_cells).
    The worlds are the survivability sweep's (sweeps._params: the default drone_radius).  Under the constant-velocity model the
    script's 121 env steps move the agents and nothing else that it reads, so only they are computed.
    `worlds`: None (built here on the host), a list of host worlds of `indices` built with sweeps._params(index), or 'device'.
    `timings`: as in traversibility_batch.  `return_agents`: also the agents [len(indices), 6, N] (a device tensor) as the
    reference's env holds them when env_metrics returns."""
    backend = _backend_of(backend, device, FIT_SCRIPT)
    t0 = time.perf_counter()
    for ix in indices:
        if ix.get('motion_profile', 'CVM') != 'CVM':
            raise NotImplementedError(f'survival_fit: motion_profile {ix["motion_profile"]!r}: only the constant-velocity model runs '
                                      f'on the device; run the reference\'s {FIT_SCRIPT}')
    plist = [sweeps._params(ix) for ix in indices]
    xs, ys = sweeps.start_cells(plist[0], position_step)
    pos = np.array([(x, y) for x in xs for y in ys], dtype=np.float64).reshape(-1, 2)
    checks = len(np.arange(0, T, 0.1))
    agents, = _seeded_worlds('survival_fit_batch', plist, worlds, backend, ('agents',))
    dev = agents.device
    if timings is not None:
        backend.sync()
    t1 = time.perf_counter()
    got = fit_first_hit(agents, torch.from_numpy(pos).to(dev), plist[0], checks, backend, return_agents)
    first, final = got if return_agents else (got, None)
    if timings is not None:
        backend.sync()
    t2 = time.perf_counter()
    host = first.cpu().numpy()
    t3 = time.perf_counter()
    times = fit_times(host.reshape(len(plist), len(xs), len(ys)), T)
    if timings is not None:
        _record(timings, dict(N=int(agents.shape[2]), worlds=len(plist), positions=len(pos), checks=checks, build_s=t1 - t0,
                              launch_s=t2 - t1, d2h_s=t3 - t2, post_s=time.perf_counter() - t3),
                ('worlds', 'build_s', 'launch_s', 'd2h_s', 'post_s'))
    return (times, final) if return_agents else times


def survival_fit(index, position_step=60, T=12, device='cuda:0', backend=None, worlds=None):
    """Drop-in for env_metrics(index) of survivability_calculator.py:13-48: np.mean of survive_times."""
    return np.mean(survival_fit_batch([index], position_step, T, device, backend, worlds)[0])


def survival_fit_table(map_ids=(0,), agent_numbers=range(10, 30, 2), agent_sizes=range(5, 15), agent_speeds=range(20, 60, 5),
                       position_step=60, T=12, device='cuda:0', backend=None, worlds=None, timings=None):
    """The nested list the reference writes to metrics_fit.csv (survivability_calculator.py:50-68), in its loop order: one row per
    map_id (the script's only one is 0), each with product(agent_num, agent_size, agent_vel) metrics.  One batch per agent count.
    `worlds`: None, 'device', or one host world per setting in that order."""
    map_ids, agent_numbers = list(map_ids), list(agent_numbers)
    order = _table_order(map_ids, agent_numbers, list(agent_sizes), list(agent_speeds))

    def batch(indices, w):
        return [np.mean(t) for t in survival_fit_batch(indices, position_step, T, device, backend, w, timings)]
    return _table('survival_fit_table', order, map_ids, agent_numbers, worlds, batch)
