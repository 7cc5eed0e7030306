"""VecDrone2DEnv — B independent Drone2D worlds stepped in lock-step on one MI355X.

Batched counterpart of the reference's `Drone2DEnv2` (envs/drone_v2.py:10-261): the same step semantics
per env, state resident in HBM, one fused HIP launch per step.  Env `i` of the batch is the world the
reference builds for `params.map_id + i` (+ `env_offset` of the shard), so results do not depend on how
the batch is sharded across GPUs.

Planner modes
  'NoMove'    traj_planner.py:68-76 runs on the device (one launch per step)
  'external'  the caller supplies plan_ok / wp_valid / wp each step (host planner plugin between
              `perceive()` and `act()`, or replayed plans with the fused `step()`)
  'Primitive' with `device_plugins=True`: traj_planner.py:78-233 runs on the device between the two halves of
              the step; with `gaze='Oxford'` yaw_planner.py:41-127 supplies the action on the device as well
              (`closed_loop()`: gaze -> perceive -> plan -> act, no host round trip); `gaze='LookAhead'` / `'LookGoal'`
              (yaw_planner.py:18-39 / :225-257) and `gaze='Owl'` (:151-222) run on the device the same way on a backend
              that has them.  `policy_step()` / `run_episodes()` drive the same stages step by step from the host
              (include/d2d_stepped.h), which is how the episodes of this planner run under motion_profile 'RVO'
  'Jerk_Primitive' with `device_plugins=True`: traj_planner.py:403-516 runs on the device between the two halves of the step
              (include/d2d_jerk.h, one launch of libd2d_jerk.so that writes plan_ok / wp_valid / wp; the planner mode stays
              'external').  `step`, `perceive` / `act`, `rollout` and `reset` run it; `closed_loop` does not (the persistent
              kernel cannot take a stage from another library).  gaze: 'external' / None (the caller's actions), 'Rotating',
              'NoControl'; on a backend with the step path's gaze launch (include/d2d_gaze.h, libd2d_gaze.so) also 'LookAhead' and
              'Owl' (yaw_planner.py:28-39, :151-222: one launch in front of the step) and 'LookGoal' and 'Oxford' (constants 0:
              this planner's trajectory is empty at every policy call).  `policy_step()` is one step of the reference's episode
              loop with the policy on the device; `run_episodes()` plays every env's episode to its end

Motion profiles (`params.motion_profile`)
  'CVM'       the agents move with their preferred velocity, inside the fused step (D2D_ST_AGENTS)
  'RVO'       utils.py:299-460: every agent first picks a velocity outside the others' reciprocal velocity obstacles
              (include/d2d_rvo.h, two launches of libd2d_rvo.so), then the fused step runs without its agents stage.
              `step`, `perceive` / `act`, `rollout` and `reset` run it; `closed_loop` does not (the persistent kernel cannot take
              a stage from another library).  `policy_step` / `run_episodes` play whole episodes under it, for the Jerk_Primitive
              planner and for the Primitive plugins; `run_episodes` moves the agents with the launches of include/d2d_rvo_live.h,
              which leave finished envs alone
"""
import numpy as np
import torch

from . import _abi as A
from . import host_init
from ._lib import D2DError, backend_for        # (importing _lib loads no library: HipBackend() does)
from .params import with_defaults
from .state import BatchState


def _build_world(args):
    params, map_id, redraw = args
    p = with_defaults(params)
    p.map_id = map_id
    return host_init.init_world(p, redraw)


def build_worlds(params, num_envs, env_offset=0, workers=0, redraw=False):
    """Host construction of `num_envs` worlds: env i is the reference world for map_id + env_offset + i.
    With `workers` > 0 the (pure Python, GPU-free) construction is spread over forked processes; call
    this before the process touches the GPU.  `redraw`: the worlds of the validation study, every agent's preferred velocity
    redrawn behind the construction (host_init.redraw_agent_velocities)."""
    p = with_defaults(params)
    jobs = [(p, p.map_id + env_offset + i, bool(redraw)) for i in range(num_envs)]
    if workers and num_envs >= 64:
        import multiprocessing as mp
        with mp.get_context('fork').Pool(workers) as pool:
            return pool.map(_build_world, jobs, chunksize=max(1, num_envs // (workers * 8)))
    return [_build_world(j) for j in jobs]


def build_worlds_of(params_list, workers=0, redraw=False):
    """One world per Params of the list (each with its own map_id and agent settings: the survivability sweep's 540 settings).
    `workers` as in build_worlds: forked processes, only before the process touches the GPU.  `redraw`: as in build_worlds."""
    jobs = [(with_defaults(p), p.map_id, bool(redraw)) for p in params_list]
    if workers and len(jobs) >= 64:
        import multiprocessing as mp
        with mp.get_context('fork').Pool(workers) as pool:
            return pool.map(_build_world, jobs, chunksize=max(1, len(jobs) // (workers * 4)))
    return [_build_world(j) for j in jobs]


def world_inputs(params_list, max_attempts=None, map_ids=None, redraw=False):
    """What the device construction (include/d2d_worlds.h) needs of `params_list`, one world each, as host arrays: the per-batch
    sizes and tables, the per-env rows, and `group` (the static map's labels, known without building anything).  Everything a
    batch shares (map, agent_number, pillar_number, static map, drone_radius, number of targets) must agree over the list.
    `map_ids`: the list is ONE Params and world i is that Params with map_ids[i] (a batch of thousands then costs no Python per env).
    `redraw`: every env's D2D_WE_REDRAW is set, the worlds of the validation study (host_init.redraw_agent_velocities)."""
    from numpy import cos, pi, sin
    plist = [with_defaults(p) for p in params_list]
    if not plist or (map_ids is not None and len(plist) != 1):
        raise ValueError('no worlds to build' if not plist else 'map_ids goes with exactly one Params')
    p0 = plist[0]
    ids = [p.map_id for p in plist] if map_ids is None else list(map_ids)

    def shared(p):
        return (tuple(p.map_size), p.map_scale, p.agent_number, p.pillar_number, str(p.static_map), p.drone_radius,
                max(len(p.target_list), 1), p.var_cam != 0)
    for i, p in enumerate(plist):
        if shared(p) != shared(p0):
            raise ValueError(f'world {i}: map, agent_number, pillar_number, static map, drone_radius, number of targets and var_cam '
                             'are per batch')
    for i, m in enumerate(ids):
        if not (isinstance(m, (int, np.integer)) and 0 <= int(m) < 2 ** 32):
            raise ValueError(f'world {i}: map_id {m!r}: numpy seeds with 0 <= map_id < 2**32 only')
    W_px, H_px, scale = int(p0.map_size[0]), int(p0.map_size[1]), int(p0.map_scale)
    if (W_px, H_px, scale) != (p0.map_size[0], p0.map_size[1], p0.map_scale):
        raise ValueError('device worlds: integer map_size and map_scale')
    n_rand, P, T = int(p0.agent_number), int(p0.pillar_number), max(len(p0.target_list), 1)
    if P and (W_px < 100 or H_px < 100):
        raise ValueError('pillars need a map of at least 100 x 100 px (randint(50, size - 50))')
    label = host_init.load_static_map(p0.static_map)
    xs, ys = np.nonzero(label)                       # x-major, as drone_v2.py:55-57 walks the map
    labs = label[xs, ys].astype(np.int64)
    if labs.size and (labs.min() < 1 or labs.max() > 99):
        raise ValueError('static map labels index the 100 drawn velocities: 0 < label < 100')
    cells = np.stack([xs, ys, labs], axis=1).astype(np.int32).reshape(-1, 3)
    unit = np.array([[cos(2 * pi * k / n_rand), sin(2 * pi * k / n_rand)] for k in range(n_rand)], dtype=np.float64).reshape(-1, 2)
    U = len(ids)
    env_par = np.zeros((len(plist), A.WORLDS_ENV_F), dtype=np.float64)
    env_tgt = np.zeros((len(plist), T, 2), dtype=np.float64)
    for i, p in enumerate(plist):
        a, b = (5, 15) if p.agent_radius == -1 else (p.agent_radius - 2, p.agent_radius + 2)
        env_par[i, [A.WE_R_LO, A.WE_R_W, A.WE_SPEED, A.WE_TRK_R]] = a, b - a, p.agent_max_speed, p.agent_radius
        env_par[i, [A.WE_X0, A.WE_Y0, A.WE_NTGT]] = p.init_position[0], p.init_position[1], len(p.target_list)
        env_par[i, A.WE_REDRAW] = 1.0 if redraw else 0.0
        for k, t in enumerate(p.target_list):
            env_tgt[i, k] = host_init._target_xy(t)
    if map_ids is not None:
        env_par, env_tgt = np.repeat(env_par, U, axis=0), np.repeat(env_tgt, U, axis=0)
    return dict(U=U, N=n_rand + len(cells), n_rand=n_rand, n_cells=len(cells), P=P, T=T, W_px=W_px, H_px=H_px, scale=scale,
                W=W_px // scale, H=H_px // scale, max_attempts=int(A.WORLDS_MAX_ATTEMPTS if max_attempts is None else max_attempts),
                start_clear=float(p0.drone_radius + 70), pillar_clear=float(p0.drone_radius + 20), unit=unit, cells=cells,
                map_id=np.array([int(m) for m in ids], dtype=np.uint64).astype(np.uint32), env_par=env_par, env_tgt=env_tgt,
                group=np.concatenate([np.zeros(n_rand, dtype=np.int64), labs]), map_ids=[int(m) for m in ids])


def world_spec(inp, grid_tile, ptr):
    """The d2d_world_spec of world_inputs() `inp`; ptr(name) is the address of array `name` where the library will read it."""
    s = A.WorldSpec()
    s.version = A.D2D_WORLDS_VERSION
    s.B = inp['U']
    for n in ('N', 'n_rand', 'n_cells', 'P', 'T', 'W_px', 'H_px', 'scale', 'W', 'H', 'max_attempts', 'start_clear', 'pillar_clear'):
        setattr(s, n, inp[n])
    s.grid_tile = int(grid_tile)
    for n in A.WORLD_SPEC_POINTERS:
        setattr(s, n, ptr(n))
    return s


def table_params(params, episodes):
    """The Params of every row of an episode table (stream_episodes(episodes=...)): a row is a Params, or a (map_id, init_position,
    target_list) triple over `params`"""
    import copy
    out = []
    for i, ep in enumerate(episodes):
        if isinstance(ep, (tuple, list)):
            if len(ep) != 3:
                raise ValueError(f'stream_episodes(): episode {i}: a row is a Params or a (map_id, init_position, target_list) triple')
            p = copy.copy(params)
            p.map_id, p.init_position, p.target_list = ep[0], ep[1], list(ep[2])
        else:
            p = with_defaults(ep)
        out.append(p)
    return out


class DeviceWorlds:
    """Seeded worlds built on the device (HipBackend.build_worlds): `state` holds the `U` distinct ones, `index` ([B] int64 on the
    device, or None) says which of them env i starts from, so a sweep's start cells share one built world.  `tracker_radius` [U, N],
    `obstacles` [U, P, 3] and `status` [U] are host copies; `group` [N] comes from the static map."""

    def __init__(self, state, index, inp, tracker_radius, obstacles, status):
        self.state, self.index = state, index
        self.N, self.T, self.U = inp['N'], inp['T'], inp['U']
        self.num_envs = self.U if index is None else int(index.numel())
        self.tracker_radius, self.obstacles, self.status = tracker_radius, obstacles, status
        self.group, self.map_ids = inp['group'], inp['map_ids']
        self.inp = inp                # (an env over these worlds rebuilds a slot of an episode table from it: stream_episodes)

    def spread(self, index):
        """The same built worlds under another env -> world index."""
        out = DeviceWorlds.__new__(DeviceWorlds)
        out.__dict__.update(self.__dict__)
        out.index = torch.as_tensor(index, dtype=torch.int64, device=self.state.device)
        out.num_envs = int(out.index.numel())
        return out


def _needs_device_worlds(backend):
    backend_for(backend, None, 'supports_device_worlds',
                'has no device world construction: build the worlds on the host (build_worlds / build_worlds_of)')


def _build_into(backend, inp, state, check=True):
    """Run the device construction of world_inputs() `inp` into BatchState `state` (B = inp['U']); returns the host copies of
    (tracker_radius, obstacles, status).  Reading them back is the call's only synchronisation."""
    _needs_device_worlds(backend)
    dev = state.device
    up = {n: torch.from_numpy(inp[n].view(np.int32) if n == 'map_id' else inp[n]).to(dev) for n in ('unit', 'cells', 'map_id', 'env_par', 'env_tgt')}
    U, N, P = inp['U'], inp['N'], inp['P']
    up['tracker_radius'] = torch.zeros((U, N), dtype=torch.float64, device=dev)
    up['obstacles'] = torch.zeros((U, P, 3), dtype=torch.int32, device=dev)
    up['status'] = torch.zeros(U, dtype=torch.int32, device=dev)
    spec = world_spec(inp, state.cfg.grid_tile, lambda n: up[n].data_ptr() if up[n].numel() else state._dummy.data_ptr())
    backend.build_worlds(spec, state.struct())
    if 'rng_draws' in state.t:
        state.t['rng_draws'].zero_()
    status = up['status'].cpu().numpy()
    if check and status.any():
        bad = np.nonzero(status)[0]
        raise D2DError(f'device worlds: env {int(bad[0])} (map_id {inp["map_ids"][int(bad[0])]}) could not place its pillars and agents '
                       f'within max_attempts = {inp["max_attempts"]} ({len(bad)} of {U} envs); the reference would loop for ever')
    return up['tracker_radius'].cpu(), up['obstacles'].cpu().numpy().astype(np.int64), status


def build_worlds_device_of(params_list, device='cuda:0', backend=None, grid_layout=None, max_attempts=None, index=None, check=True,
                           map_ids=None, redraw=False):
    """build_worlds_of on the device: one world per Params of the list, built by one launch and left resident (DeviceWorlds).
    `index`: env -> position in the list, for batches that start many envs from one world.  `check=False` returns instead of raising
    D2DError when an env hit `max_attempts` (DeviceWorlds.status says which; their fields are 0).  `map_ids`, `redraw`: as in
    world_inputs."""
    backend = backend_for(backend, device)
    inp = world_inputs(params_list, max_attempts, map_ids, redraw)
    p0 = with_defaults(params_list[0])
    cfg = host_init.derive_cfg(p0, B=inp['U'], N=inp['N'], T=inp['T'], grid_tile=_grid_tile(p0, backend, grid_layout))
    state = BatchState(cfg, torch.device(backend.device))
    tr, obs, status = _build_into(backend, inp, state, check)
    idx = None if index is None else torch.as_tensor(index, dtype=torch.int64, device=state.device)
    return DeviceWorlds(state, idx, inp, tr, obs, status)


def build_worlds_device(params, num_envs, env_offset=0, device='cuda:0', backend=None, grid_layout=None, max_attempts=None, check=True,
                        redraw=False):
    """build_worlds on the device: env i is the reference world for map_id + env_offset + i."""
    return build_worlds_device_of([params], device, backend, grid_layout, max_attempts, check=check,
                                  map_ids=_seeded(params, num_envs, env_offset), redraw=redraw)


def _seeded(params, num_envs, env_offset):
    m0 = with_defaults(params).map_id + env_offset
    return [m0 + i for i in range(num_envs)]


def _grid_tile(params, backend, grid_layout):
    """d2d_cfg.grid_tile of `grid_layout` ('rowmajor' = the reference's [W][H]; 'tiled' = 16 x 16-cell tiles).  Default: tiled on the
    HIP backend for grids above 256 x 256 cells (BASELINE config 5: a 3 x 3 block or a 23-byte window row of a 640-cell row-major
    grid costs a cache line each), row-major otherwise; `state.logical()` / the facade proxies always speak [W][H]."""
    W, H = params.map_size[0] // params.map_scale, params.map_size[1] // params.map_scale
    if grid_layout is None:
        grid_layout = 'tiled' if (W * H > 256 * 256 and getattr(backend, 'supports_tiled_grids', False)) else 'rowmajor'
    if grid_layout not in ('rowmajor', 'tiled'):
        raise ValueError(f'grid_layout {grid_layout!r}: rowmajor or tiled')
    return 16 if grid_layout == 'tiled' else 0


class VecDrone2DEnv:
    def __init__(self, params, num_envs, device='cuda:0', planner=None, env_offset=0, backend=None,
                 kf_enabled=True, worlds=None, device_plugins=False, gaze=None, grid_layout=None, jerk_tie=None, redraw_agents=False,
                 swept_obs=False, seen_obs=False, scan_obs=False, tracks_obs=False, tracks_samples=31, tracks_margin=None):
        """`jerk_tie`: (tie_perm, tie_eq) for planner='Jerk_Primitive' in place of the table of this host's np.argsort
        (jerk_plugin.tie_table): a recorded episode replays with the table of the numpy that recorded it.
        `redraw_agents`: the worlds this env builds itself (worlds=None, worlds='device') are those of the validation study: every
        agent's preferred velocity redrawn behind the construction (host_init.redraw_agent_velocities, D2D_WE_REDRAW).  The reset
        snapshot is taken behind the redraw, so reset() and closed_loop(auto_reset=True) restore the redrawn world, as the script's
        env.reset() and redraw do.  Worlds handed over are taken as they are: build them with `redraw=`.
        `swept_obs`: obs['swep_map'] is the crop of the map Primitive.replan_check returned in the step (the cells the stored
        trajectory will pass through and when: envs/training_v3.py:141, :206-213, include/d2d_swept.h) instead of the explored map a
        second time (envs/drone_v2.py:252-253); `swept_map` and `swept_count` hold the full map and the waypoints marked.  The env then
        steps through policy_step() / run_episodes() / action_stream() and stream_episodes(), one launch per stage.
        `seen_obs`: obs['age_map'] [B, 1, L, L] float32 is the crop of the time-since-observed map, what yaw_planner.Oxford keeps as
        last_time_observed_map (yaw_planner.py:49, :92-97) and decides from, for the pose the env is in now, whichever planner and
        gaze run (include/d2d_seen.h); `seen_calls`, `seen_age` and `refreshed` hold the full map and the cells the pose newly
        covered.  One more launch behind every single step; closed_loop() and rollout(), whose steps nobody sees, refuse it.
        `scan_obs`: obs['scan'] [B, 2, R] float32 is the sensor's own reading, one range and one outcome per ray of the step's
        raycast (include/d2d_scan.h); `ray_end`, `ray_kind` and `ray_hits` hold what the reference keeps as env.drone.rays
        (utils.py:712, :746), bit for bit but for 'wall' at a range stop, which is 2 where the reference has the raw map_gt value (2,
        or 3 on a cell that still carries the previous step's dynamic mark).  A copy of the pose in front of every single step and
        one more launch behind it; no rays before the first step; closed_loop(n > 1) and rollout() refuse it.
        `tracks_obs`: obs['track_map'] [B, 1, L, L] float32 is the window around the drone of the tracker-forecast map
        (include/d2d_tracks.h): 1 + the first of the samples k = 0 .. tracks_samples - 1 (1 .. 255; 31 is k * dt up to 3 s, Oxford's
        tau_s, yaw_planner.py:55) at which an active Kalman tracker's estimate_pos(k * dt) comes within drone_radius +
        tracker.radius + tracks_margin of the cell's centre, 0 where none does.  `tracks_margin` None is 5 + var_cam, the keep-out
        of Planner.is_free (traj_planner.py:57); 0 is the test of replan_check (:227).  `track_win` and `track_cells` hold the
        uint8 window and its nonzero cells.  The radii are the device planner's (planner 'Primitive' or 'Jerk_Primitive' with
        device_plugins=True).  One more launch behind every single step and reset(); closed_loop() and rollout() refuse it."""
        self.params = with_defaults(params)
        # the arguments as given: sibling() builds a second env from them
        self._ctor = dict(params=params, device=device, planner=planner, env_offset=env_offset, backend=backend, kf_enabled=kf_enabled,
                          worlds=worlds, device_plugins=device_plugins, gaze=gaze, grid_layout=grid_layout, jerk_tie=jerk_tie,
                          redraw_agents=redraw_agents, swept_obs=swept_obs, seen_obs=seen_obs, scan_obs=scan_obs, tracks_obs=tracks_obs,
                          tracks_samples=tracks_samples, tracks_margin=tracks_margin)
        self._action_stream = None         # the open action_stream.ActionStream over this env, or None
        self.redraw_agents = bool(redraw_agents)
        self.num_envs = int(num_envs)
        self.env_offset = int(env_offset)
        planner = planner if planner is not None else self.params.planner
        self.planner_mode = A.PLANNER_NOMOVE if planner == 'NoMove' else A.PLANNER_EXTERNAL
        profile = self.params.motion_profile
        if profile not in ('CVM', 'RVO'):
            raise ValueError(f"motion_profile {profile!r}: 'CVM' or 'RVO'")
        self.rvo = profile == 'RVO'
        if self.rvo and (self.params.agent_max_speed == 0 or self.params.agent_radius == -1):
            # np.arange(0.02, 0 + 0.02, 0 / 5.0) raises in the reference's intersect(), outside RVO_update's try (utils.py:367)
            raise NotImplementedError("motion_profile 'RVO' with agent_max_speed == 0 or agent_radius == -1: the reference itself "
                                      'cannot run RVO with these parameters')
        self.backend = backend = backend_for(backend, device)
        if self.rvo:
            backend_for(backend, device, 'supports_rvo', "has no RVO motion profile (motion_profile='RVO' runs on the HIP backend)")
        self.device = torch.device(backend.device)
        # worlds='device' / a DeviceWorlds: the seeded worlds are built by the device (include/d2d_worlds.h) and never exist on the host;
        # N and T follow from the parameters and the static map
        dw = worlds if isinstance(worlds, DeviceWorlds) else None
        on_device = dw is not None or (isinstance(worlds, str) and worlds == 'device')
        if isinstance(worlds, str) and not on_device:
            raise ValueError(f"worlds {worlds!r}: a list of host worlds, a DeviceWorlds or 'device'")
        if on_device:
            _needs_device_worlds(backend)
            inp = None if dw is not None else world_inputs([self.params], map_ids=_seeded(self.params, self.num_envs, self.env_offset),
                                                           redraw=self.redraw_agents)
            N, T = (dw.N, dw.T) if dw is not None else (inp['N'], inp['T'])
            if dw is not None and dw.num_envs != self.num_envs:
                raise ValueError(f'{dw.num_envs} device worlds for {self.num_envs} envs')
        else:
            if worlds is None:
                worlds = build_worlds(self.params, self.num_envs, self.env_offset, workers=0, redraw=self.redraw_agents)
            N = worlds[0]['N'] if worlds else 0
            T = worlds[0]['T'] if worlds else 1
            if any(w['N'] != N for w in worlds):
                raise ValueError('all envs of a batch must have the same number of agents')
        self._world_inp = inp if on_device and dw is None else None     # what stream_episodes() rebuilds a slot's world from
        # ... and what stream_episodes(episodes=...) rebuilds it from where the worlds were handed over, one built world per env
        self._table_inp = self._world_inp if dw is None else (dw.inp if dw.index is None and hasattr(dw, 'inp') else None)
        self._streamed = False
        self._own_noise = False
        self.cfg = host_init.derive_cfg(self.params, B=self.num_envs, N=N, T=T, planner_mode=self.planner_mode,
                                        kf_enabled=kf_enabled, grid_tile=_grid_tile(self.params, backend, grid_layout))
        self.state = BatchState(self.cfg, self.device)
        if dw is not None:
            self.state.load_device_worlds(dw)
            self.tracker_radius = dw.tracker_radius if dw.index is None else dw.tracker_radius[dw.index.cpu()]
            pillars = dw.obstacles if dw.index is None else dw.obstacles[dw.index.cpu().numpy()]
        elif on_device:
            self.tracker_radius, pillars = _build_into(backend, inp, self.state)[:2] if self.num_envs else (None, np.zeros((0, 0, 3)))
        else:
            self.state.load_worlds(worlds)
            pillars = None
            if self.rvo:                       # (worlds built by hand for the constant-velocity model need not name their pillars)
                if len({len(w['obstacles']) for w in worlds}) > 1:
                    raise ValueError("motion_profile 'RVO': all envs of a batch must have the same number of pillars")
                pillars = np.stack([w['obstacles'] for w in worlds]) if worlds else np.zeros((0, 0, 3))
            if worlds:
                from .state import distinct_worlds
                distinct, index = distinct_worlds(worlds)
                self.tracker_radius = torch.from_numpy(np.stack([w['tracker_radius'] for w in distinct]))[torch.as_tensor(index)]
            else:
                self.tracker_radius = None
        if self.rvo:
            self.state.init_rvo(min(int(self.params.agent_number), N), pillars, np.asarray(pillars).shape[1] if self.num_envs else self.params.pillar_number)
        else:
            # the pillars stay resident under either motion profile: the renderer draws them (include/d2d_render.h), and as a tensor
            # of state.t they follow a slot through load_slots() and a stream's refill.  Host worlds built by hand that do not name
            # theirs (or not the same number each) keep none, and none is drawn
            if pillars is None:
                named = [np.asarray(w['obstacles']).reshape(-1, 3) for w in worlds if 'obstacles' in w]
                if len(named) == len(worlds) and len({len(o) for o in named}) <= 1:
                    pillars = np.stack(named) if named else np.zeros((0, 0, 3))
            if pillars is not None:
                self.state.init_pillars(pillars, np.asarray(pillars).shape[1] if self.num_envs else self.params.pillar_number)
        self.init_state = self.state.clone_world()
        self._st = self.state.struct()
        self._init_st = self.init_state.struct()
        # var_cam != 0: the tracker stage draws the measurement noise from the env's own stream (d2d_state.rng) unless set_noise()
        # supplies the draws; a backend without that stage sees no stream and refuses the step until it gets them
        self.device_noise = 'rng' in self.state.t and bool(getattr(backend, 'supports_device_noise', False))
        if not self.device_noise:
            for st in (self._st, self._init_st):
                st.rng = st.rng_draws = None
        self.reward = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)   # drone_v2.py:257
        self.plugins = None
        self.jerk = None
        self.gaze_state = None             # gaze_plugin.GazeState: LookAhead / Owl as a launch in front of the step
        self.step_gaze = None              # the gaze policy the step path evaluates itself (policy_step, run_episodes), or None
        self.device_gaze = None            # the gaze policy the device evaluates in whichever loop runs the episodes, or None
        if device_plugins and planner == 'Jerk_Primitive':
            # its own library and its own per-batch state (jerk_plugin.JerkState): no d2d_plan is involved
            # LookAhead / Owl: a launch of libd2d_gaze.so in front of the step (include/d2d_gaze.h), on a backend that has it.
            # LookGoal / Oxford: this planner's trajectory is empty at every policy call (plan() appends one waypoint, step_pos pops
            # it), and both policies answer 0 for an empty trajectory (yaw_planner.py:235-236, :117-118): resident constants
            step_gaze = bool(getattr(backend, 'supports_step_gaze', False))
            if gaze not in ('external', None, 'Rotating', 'NoControl') and not step_gaze:
                raise NotImplementedError(f"device plugins: planner 'Jerk_Primitive' / gaze {gaze!r}: the device Jerk_Primitive planner "
                                          "takes gaze 'external' (the caller's actions), 'Rotating' or 'NoControl'; drive any other "
                                          'policy from the host (gaze.LookAhead, ...) and pass its actions to step()')
            if gaze not in ('external', None, 'Rotating', 'NoControl', 'LookAhead', 'Owl', 'LookGoal', 'Oxford'):
                raise NotImplementedError(f"device plugins: planner 'Jerk_Primitive' / gaze {gaze!r}: the device Jerk_Primitive planner "
                                          "takes gaze 'external' (the caller's actions), 'Rotating', 'NoControl', 'LookAhead', 'Owl', "
                                          "'LookGoal' or 'Oxford'; drive any other policy from the host and pass its actions to step()")
            backend_for(backend, device, 'supports_jerk', "has no Jerk_Primitive planner (planner='Jerk_Primitive' with "
                        'device_plugins=True runs on the HIP backend)')
            if not kf_enabled and N:
                raise ValueError("device plugins: planner 'Jerk_Primitive' reads the Kalman trackers (kf_enabled=True)")
            from .jerk_plugin import JerkState
            self.jerk = JerkState(self.params, self.cfg, self.device, self.tracker_radius.numpy() if N and self.num_envs else None,
                                  tie=jerk_tie)
            self._jerk_call = self.jerk.call(self.state)
            if gaze in ('Rotating', 'NoControl', 'LookGoal', 'Oxford'):
                self.state.action.fill_(1.0 if gaze == 'Rotating' else 0.0)
            elif gaze in ('LookAhead', 'Owl'):
                from .gaze_plugin import GazeState
                self.gaze_state = GazeState(self.params, self.cfg, self.device, gaze)
                self._gaze_call = self.gaze_state.call(self.state)
            self.step_gaze = self.device_gaze = gaze if gaze not in ('external', None) else None
        elif device_plugins:
            from .device_plugins import PluginState
            gaze = gaze if gaze is not None else self.params.gaze_method
            if planner not in ('Primitive', 'NoMove') or gaze not in ('Oxford', 'LookAhead', 'LookGoal', 'Owl', 'Rotating', 'NoControl',
                                                                      'external', None):
                raise NotImplementedError(f'device plugins: planner {planner!r} / gaze {gaze!r} '
                                          '(device: Primitive, NoMove / Oxford, LookAhead, LookGoal, Owl, Rotating, NoControl)')
            # LookAhead / LookGoal (yaw_planner.py:18-39, :225-257) call math.atan2: only a backend with the bit-exact device
            # restatement runs them as a gaze stage (under NoMove LookGoal sees no trajectory and returns 0, as the reference does)
            if gaze in ('LookAhead', 'LookGoal') and not getattr(self.backend, 'supports_device_heading_gaze', False):
                raise NotImplementedError(f'device plugins: gaze {gaze!r} needs a backend with the device LookAhead / LookGoal stage '
                                          f'({getattr(self.backend, "name", type(self.backend).__name__)} has none); drive the '
                                          "policy from the host with gaze='external' and gaze.LookAhead / gaze.LookGoal")
            # Owl (yaw_planner.py:151-222) needs libm's pow(x, 2.0) bit for bit as well, and its own per-env state
            if gaze == 'Owl' and not getattr(self.backend, 'supports_device_owl_gaze', False):
                raise NotImplementedError(f"device plugins: gaze 'Owl' needs a backend with the device Owl stage "
                                          f'({getattr(self.backend, "name", type(self.backend).__name__)} has none); drive the '
                                          "policy from the host with gaze='external' and gaze.Owl")
            if gaze == 'Owl' and not kf_enabled:
                raise ValueError("device plugins: gaze 'Owl' reads the Kalman trackers (kf_enabled=True)")
            self.plugins = PluginState(self.params, self.cfg, self.device, self.tracker_radius.numpy(),
                                       planner=planner, gaze=gaze or 'external')
            self._plan = self.plugins.struct()
            # the constant policies of the reference need no kernel: Rotating.plan -> 1 (yaw_planner.py:136-142),
            # NoControl.plan -> 0 (:10-16); the action stays resident
            if gaze == 'Rotating':
                self.state.action.fill_(1.0)
            elif gaze == 'NoControl':
                self.state.action.fill_(0.0)
            # the step path's episode loop (policy_step, run_episodes) takes the Primitive plugins with a policy of their own
            if planner == 'Primitive' and gaze not in ('external', None):
                self.step_gaze = gaze
            self.device_gaze = gaze if gaze not in ('external', None) else None
        self.swept_obs = bool(swept_obs)
        self.swept = None                  # the buffers of include/d2d_swept.h (Jerk_Primitive: the crop alone, zero for ever)
        if self.swept_obs:
            self._init_swept(planner)
        self.seen_obs = bool(seen_obs)
        self.seen = None                   # the buffers of include/d2d_seen.h
        if self.seen_obs:
            self._init_seen()
        self.scan_obs = bool(scan_obs)
        self.scan = None                   # the buffers of include/d2d_scan.h
        if self.scan_obs:
            self._init_scan()
        self.tracks_obs = bool(tracks_obs)
        self.tracks = None                 # the buffers of include/d2d_tracks.h
        if self.tracks_obs:
            self._init_tracks(planner, kf_enabled, tracks_samples, tracks_margin)

    def _init_swept(self, planner):
        """The refusals and the buffers of swept_obs=True"""
        if self.plugins is None and self.jerk is None:
            raise RuntimeError('swept_obs=True needs device_plugins=True: the swept map is what the device planner\'s replan_check '
                               "returns (planner='Primitive' or 'Jerk_Primitive')")
        if self.jerk is None and self.plugins.planner != A.PLAN_PRIMITIVE:
            raise NotImplementedError(f"swept_obs=True: planner {planner!r} has no swept map of its own -- NoMove.replan_check returns "
                                      "the explored map itself (traj_planner.py:75-76), which obs['local_map'] already crops; the "
                                      "device computes it for planner='Primitive' (and zeros for 'Jerk_Primitive')")
        backend_for(self.backend, None, 'supports_swept_obs', 'has no swept-map launches (include/d2d_swept.h: d2d_swept_mark, '
                    'd2d_swept_crop): swept_obs=True runs on a HIP library built with them')
        if self.cfg.W > A.SWEPT_MAX_SIDE or self.cfg.H > A.SWEPT_MAX_SIDE:
            raise NotImplementedError(f'swept_obs=True: a map of {self.cfg.W} x {self.cfg.H} cells; the stage holds an env\'s map in LDS '
                                      f'whole and takes at most {A.SWEPT_MAX_SIDE} x {A.SWEPT_MAX_SIDE} (the channel would cost '
                                      f'{self.cfg.W * self.cfg.H} bytes per env and step)')
        B, L, dev = self.num_envs, self.cfg.L, self.device
        self.swept = {'obs': torch.zeros((B, L, L), dtype=torch.uint8, device=dev)}
        if self.jerk is not None:          # an empty trajectory at every replan_check (plan() appends one waypoint, step_pos pops it)
            return
        self.swept.update(map=torch.zeros_like(self.state.dmap), count=torch.zeros(B, dtype=torch.int32, device=dev),
                          live=torch.zeros(B, dtype=torch.uint8, device=dev))
        self._swept = A.Swept()
        for n in A.SWEPT_FIELDS:
            t = self.swept[n]
            setattr(self._swept, n, t.data_ptr() if t.numel() else self.state._dummy.data_ptr())

    @property
    def swept_map(self):
        """[B, W, H] uint8: the map replan_check returned in each env's last live step (None under Jerk_Primitive: all zero)"""
        if not self.swept_obs:
            raise RuntimeError('swept_map: build the env with swept_obs=True')
        m = self.swept.get('map')
        if m is not None and self.cfg.grid_tile:
            from .state import untile_grid
            return untile_grid(m, self.cfg.W, self.cfg.H, self.cfg.grid_tile)
        return m

    @property
    def swept_count(self):
        """[B] int32: the waypoints marked in that map (first tracker hit + 1, or the trajectory's length)"""
        if not self.swept_obs:
            raise RuntimeError('swept_count: build the env with swept_obs=True')
        return self.swept.get('count')

    def _swept_zero(self, mask=None):
        """map, crop and count of a fresh world (envs/training_v3.py:219-224), for all envs or those of `mask`"""
        if self.swept is None or len(self.swept) == 1:
            return
        for t in self.swept.values():
            if mask is None:
                t.zero_()
            elif t.numel():
                t.masked_fill_(mask.bool().view((-1,) + (1,) * (t.dim() - 1)), 0)

    def _init_seen(self):
        """The refusals and the buffers of seen_obs=True, and the update of call 1: the map as the start pose sees it"""
        import math
        from .device_plugins import acos_window, tobs_table
        backend_for(self.backend, None, 'supports_seen_obs', 'has no time-since-observed launch (include/d2d_seen.h: d2d_seen_update): '
                    'seen_obs=True runs on the HIP backend, with csrc/seen/libd2d_seen.so built')
        key_lo, mask = acos_window(math.radians(self.params.drone_view_range / 2))      # raises for a view range it cannot describe
        B, L, dev = self.num_envs, self.cfg.L, self.device
        tab = tobs_table(self.params)
        i32 = torch.int32
        self.seen = dict(seen=torch.zeros((B, self.cfg.W, self.cfg.H), dtype=i32, device=dev), last_call=torch.zeros(B, dtype=i32, device=dev),
                         refreshed=torch.zeros(B, dtype=i32, device=dev), obs=torch.zeros((B, L, L), dtype=torch.float32, device=dev),
                         tab=torch.from_numpy(tab).to(dev))
        self._seen = A.Seen()
        for n in A.SEEN_POINTERS:
            t = self.seen[n]
            setattr(self._seen, n, t.data_ptr() if t.numel() else self.state._dummy.data_ptr())
        self._seen.acos_key_lo, self._seen.acos_mask, self._seen.tab_len, self._seen.reserved = key_lo, mask, tab.shape[1], 0
        self._seen_update()

    def _seen_update(self):
        """d2d_seen_update: every env whose step counter has moved since its latest update (or that was zeroed) marks what its
        pose sees and crops; a finished env, whose counter stands still, is left as it is"""
        if self.seen is not None and self.num_envs:
            self.backend.seen_update(self.cfg, self._st, self._seen)

    def _seen_zero(self, mask=None):
        """the map of a fresh world (Oxford.__init__, yaw_planner.py:49: nothing seen yet) for all envs or those of `mask`, then the
        update of call 1 from the start pose; the other envs' calls have not moved, so the launch leaves them alone"""
        if self.seen is None:
            return
        for n in ('seen', 'last_call'):
            t = self.seen[n]
            if mask is None:
                t.zero_()
            elif t.numel():
                t.masked_fill_(mask.bool().view((-1,) + (1,) * (t.dim() - 1)), 0)
        self._seen_update()

    def _seen_needed(self, what):
        if not self.seen_obs:
            raise RuntimeError(f'{what}: build the env with seen_obs=True')

    @property
    def seen_calls(self):
        """[B, W, H] int32: the number of the Oxford.plan() call (steps taken + 1) that last saw each cell, 0 = never"""
        self._seen_needed('seen_calls')
        return self.seen['seen']

    @property
    def seen_age(self):
        """[B, W, H] float64: Oxford.last_time_observed_map as of each env's latest update, gathered from the table of the
        reference's own additions (device_plugins.tobs_table)"""
        self._seen_needed('seen_age')
        sn, call, tab = self.seen['seen'].long(), self.seen['last_call'].long()[:, None, None], self.seen['tab']
        return torch.where(sn > 0, tab[0][call - torch.minimum(sn.clamp(min=0), call)], tab[1][call.expand_as(sn)])

    @property
    def refreshed(self):
        """[B] int32: the cells each env's latest update marked that the call before had not seen"""
        self._seen_needed('refreshed')
        return self.seen['refreshed']

    def _init_scan(self):
        """The refusal and the buffers of scan_obs=True.  No launch: a fresh world has no rays yet (utils.py:726, `self.rays = {}`)"""
        backend_for(self.backend, None, 'supports_scan_obs', 'has no per-ray scan launch (include/d2d_scan.h: d2d_scan_update): '
                    'scan_obs=True runs on the HIP backend, with csrc/scan/libd2d_scan.so built')
        B, R, dev = self.num_envs, self.cfg.R, self.device
        words = max(1, (self.cfg.N + 31) // 32)
        self.scan = dict(pose=torch.zeros((B, A.DF), dtype=torch.float64, device=dev), end=torch.zeros((B, R, 2), dtype=torch.float64, device=dev),
                         kind=torch.zeros((B, R), dtype=torch.uint8, device=dev), hit=torch.zeros((B, R, words), dtype=torch.int32, device=dev),
                         obs=torch.zeros((B, 2, R), dtype=torch.float32, device=dev), last_step=torch.zeros(B, dtype=torch.int32, device=dev))
        self._scan = A.Scan()
        for n in A.SCAN_POINTERS:
            t = self.scan[n]
            setattr(self._scan, n, t.data_ptr() if t.numel() else self.state._dummy.data_ptr())
        self._scan.hit_words, self._scan.reserved = words, 0

    def _scan_snapshot(self):
        """the pose the coming step's rays are cast from (drone_v2.py:173 runs before step_pos / step_yaw): queued in front of the
        step's first launch"""
        if self.scan is not None:
            self.scan['pose'].copy_(self.state.drone)

    def _scan_update(self):
        """d2d_scan_update: every env whose step counter has moved since its latest update gets the rays of that step; a finished
        env, whose counter stands still, and a world that has not stepped are left as they are"""
        if self.scan is not None and self.num_envs:
            self.backend.scan_update(self.cfg, self._st, self._scan)

    def _scan_zero(self, mask=None):
        """no rays yet (utils.py:726) for all envs or those of `mask`: a slot whose previous episode ended at step k would otherwise
        be skipped at step k of its next one"""
        if self.scan is None:
            return
        for n in A.SCAN_OUTPUTS:
            t = self.scan[n]
            if mask is None:
                t.zero_()
            elif t.numel():
                t.masked_fill_(mask.bool().view((-1,) + (1,) * (t.dim() - 1)), 0)

    def _scan_needed(self, what):
        if not self.scan_obs:
            raise RuntimeError(f'{what}: build the env with scan_obs=True')

    @property
    def ray_end(self):
        """[B, R, 2] float64: 'coords' of every ray of the latest step (utils.py:712), (-1, -1) where the ray did not stop"""
        self._scan_needed('ray_end')
        return self.scan['end']

    @property
    def ray_kind(self):
        """[B, R] uint8: 0 no stop, 1 an OCCUPIED cell, 2 inside an agent, 3 the range (include/d2d_scan.h)"""
        self._scan_needed('ray_kind')
        return self.scan['kind']

    @property
    def ray_hits(self):
        """[B, R, N] bool: 'hit_list' of every ray, unpacked from the words on demand"""
        self._scan_needed('ray_hits')
        h = self.scan['hit']
        bits = (h.unsqueeze(-1) >> torch.arange(32, dtype=torch.int32, device=h.device)) & 1
        return bits.reshape(h.shape[0], h.shape[1], -1)[:, :, :self.cfg.N].bool()

    def _init_tracks(self, planner, kf_enabled, samples, margin):
        """The refusals and the buffers of tracks_obs=True, and the first update: a fresh world has no active tracker (utils.py:182)"""
        if not 1 <= int(samples) <= A.TRACKS_MAX_SAMPLES:
            raise ValueError(f'tracks_obs=True: tracks_samples={samples!r} (1 .. {A.TRACKS_MAX_SAMPLES}: the window holds 1 + the sample '
                             'as a uint8)')
        if not kf_enabled:
            raise ValueError('tracks_obs=True reads the Kalman trackers (kf_enabled=True)')
        radii = self.jerk.t['trk_radius'] if self.jerk is not None else \
            self.plugins.t['trk_radius'] if self.plugins is not None and self.plugins.planner == A.PLAN_PRIMITIVE else None
        if radii is None:
            raise NotImplementedError(f"tracks_obs=True: planner {planner!r} {'with' if self.plugins is not None else 'without'} device "
                                      'plugins keeps no tracker radii (trk_radius, envs/drone_v2.py:46, utils.py:239: the device '
                                      "planners' d2d_plan.trk_radius / d2d_jerk_call.trk_radius); build the env with planner='Primitive' "
                                      "or 'Jerk_Primitive' and device_plugins=True")
        backend_for(self.backend, None, 'supports_tracks_obs', 'has no tracker-forecast launch (include/d2d_tracks.h: d2d_tracks_update): '
                    'tracks_obs=True runs on the HIP backend, with csrc/tracks/libd2d_tracks.so built')
        B, L, dev = self.num_envs, self.cfg.L, self.device
        self.tracks = dict(trk_radius=radii, win=torch.zeros((B, L, L), dtype=torch.uint8, device=dev),
                           cells=torch.zeros(B, dtype=torch.int32, device=dev), last_step=torch.full((B,), -1, dtype=torch.int32, device=dev),
                           obs=torch.zeros((B, L, L), dtype=torch.float32, device=dev))
        self._tracks = A.Tracks()
        for n in A.TRACKS_POINTERS:
            t = self.tracks[n]
            setattr(self._tracks, n, t.data_ptr() if t.numel() else self.state._dummy.data_ptr())
        self._tracks.margin = float(5 + self.params.var_cam if margin is None else margin)
        self._tracks.samples, self._tracks.force = int(samples), 0
        self._tracks_update()

    def _tracks_update(self):
        """d2d_tracks_update: every env whose step counter differs from that of its latest update gets its window; a finished env,
        whose counter stands still, is left as it is, and a reset or refilled slot, which has no active tracker, comes out zero"""
        if self.tracks is not None and self.num_envs:
            self.backend.tracks_update(self.cfg, self._st, self._tracks)
            self.tracks['obs'].copy_(self.tracks['win'])       # obs['track_map']: the same values as float32, resident

    def tracks_refresh(self):
        """The window of every env from the state as it stands, whatever the step counters say: for a caller that writes the drone,
        the trackers or the radii itself"""
        self._tracks_needed('tracks_refresh()')
        self._tracks.force = 1
        try:
            self._tracks_update()
        finally:
            self._tracks.force = 0

    def _tracks_needed(self, what):
        if not self.tracks_obs:
            raise RuntimeError(f'{what}: build the env with tracks_obs=True')

    @property
    def track_win(self):
        """[B, L, L] uint8: the window of the tracker-forecast map, 1 + the first sample that reaches the cell, 0 = none"""
        self._tracks_needed('track_win')
        return self.tracks['win']

    @property
    def track_cells(self):
        """[B] int32: the nonzero cells of each env's window"""
        self._tracks_needed('track_cells')
        return self.tracks['cells']

    # ------------------------------------------------------------------ gym-like surface (batched)
    @property
    def N(self):
        return self.cfg.N

    def reset(self, mask=None):
        """envs/drone_v2.py:259-261: back to the seeded initial world (all envs, or those in `mask`)."""
        if self._streamed:
            raise RuntimeError('reset(): this env has streamed episodes (stream_episodes), so its slots hold other worlds than its '
                               'snapshot; build a new VecDrone2DEnv for the map ids you want')
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self.backend.reset(self.cfg, self._st, self._init_st, mask)
        if self.rvo:
            vel, vel0 = self.state.agent_vel, self.init_state.agent_vel
            vel.copy_(vel0 if mask is None else torch.where(mask.bool()[:, None, None], vel0, vel))
        self.reset_plugins(mask)
        self._swept_zero(mask)
        self._seen_zero(mask)
        self._scan_zero(mask)
        self._tracks_update()              # (a reset env's counter jumped back: its window comes out zero)
        return {}

    def _rvo_agents(self):
        """RVO_update + Agent.step of every env (include/d2d_rvo.h): the decisions read the positions and velocities of before the
        step, so they are a launch of their own; the velocity buffers swap afterwards."""
        s = self.state
        if self.num_envs == 0:
            return
        self.backend.rvo_velocity(s.agents, s.agent_vel, s.pillars, s.agent_vel_out)
        self.backend.rvo_agents_step(s.agents, s.agent_vel_out, self.cfg.W_px, self.cfg.H_px, self.cfg.scale, self.cfg.dt)
        s.t['agent_vel'], s.t['agent_vel_out'] = s.t['agent_vel_out'], s.t['agent_vel']

    def _rvo_agents_live(self):
        """_rvo_agents for the envs that are not done (include/d2d_rvo_live.h): a finished env's agents stay where they are, and its
        velocities go through the swap unchanged"""
        s = self.state
        if self.num_envs == 0:
            return
        self.backend.rvo_velocity_live(s.agents, s.agent_vel, s.pillars, s.flags, s.agent_vel_out)
        self.backend.rvo_agents_step_live(s.agents, s.agent_vel_out, s.flags, self.cfg.W_px, self.cfg.H_px, self.cfg.scale, self.cfg.dt)
        s.t['agent_vel'], s.t['agent_vel_out'] = s.t['agent_vel_out'], s.t['agent_vel']

    def run_step(self):
        """d2d_step with the action already set; under RVO the agents move first, then every other stage (the state machine stage,
        which d2d_step runs before the agents, does not touch them: the order is the reference's)"""
        self._scan_snapshot()
        if self.jerk is not None:
            self.run_perceive()
            self.run_jerk_plan()
            self.backend.act(self.cfg, self._st)
        elif self.rvo:
            self._rvo_agents()
            self.backend.run_stages(self.cfg, self._st, A.ST_ALL & ~A.ST_AGENTS)
        else:
            self.backend.step(self.cfg, self._st)
        self._seen_update()
        self._scan_update()
        self._tracks_update()

    def run_gaze(self):
        """d2d_gaze_act for every env that is not done: the action of the coming step, from what the previous step left.  The
        constant policies (Rotating, NoControl; LookGoal and Oxford under Jerk_Primitive) keep their resident action"""
        if self.gaze_state is not None and self.num_envs:
            self.backend.gaze_act(self._gaze_call)

    def _needs_step_gaze(self, what):
        if self.step_gaze is None:
            raise RuntimeError(f"{what} needs planner='Jerk_Primitive' or 'Primitive', device_plugins=True and a gaze policy the step "
                               "path evaluates: 'LookAhead', 'Owl', 'LookGoal', 'Oxford', 'Rotating' or 'NoControl'")
        if self.plugins is not None:
            backend_for(self.backend, None, 'supports_stepped_plugins', f'has no gaze and plan stages that leave finished envs alone '
                        f'(include/d2d_stepped.h): {what} with the Primitive plugins runs on the HIP backend')
            if self.rvo:
                backend_for(self.backend, None, 'supports_rvo_live', f'has no RVO launches that leave finished envs alone '
                            f'(include/d2d_rvo_live.h): {what} with the Primitive plugins under RVO runs on the HIP backend')

    def _jerk_live(self, live):
        """Does run_episodes() with planner='Jerk_Primitive' take the launches that leave finished envs alone?  `live` None: where
        the backend has them; True: they are required; False: no"""
        if live is not None and not live:
            return False
        lacks = [(flag, what) for flag, what, needed in (
            ('supports_jerk_live', 'has no plan launch that leaves finished envs alone (include/d2d_jerk_live.h)', True),
            ('supports_rvo_live', 'has no RVO launches that leave finished envs alone (include/d2d_rvo_live.h)', self.rvo))
            if needed and not getattr(self.backend, flag, False)]
        if lacks and live:
            backend_for(self.backend, None, lacks[0][0], f"{lacks[0][1]}: run_episodes(live=True) with planner 'Jerk_Primitive'"
                        f"{' under RVO' if self.rvo else ''} runs on the HIP backend")
        return not lacks

    def _plugins_step(self, before_plan=None):
        """One step of the episode loop with the Primitive plugins, finished envs left alone by every launch: d2d_gaze_stage_live
        (nothing for the resident constants), under RVO the two _live RVO launches, d2d_run_stages(PERCEIVE | SKIP_DONE) with this
        step's row of the noise, d2d_plan_stage_live, d2d_run_stages(ACT | SKIP_DONE).  The gaze decision reads the drone, the
        trajectory, seen_step and the trackers, none of which the RVO launches write, so the order is the reference's: policy.plan,
        then step() with the agents first.  With swept_obs d2d_swept_mark goes between the perceive and the plan launch (the
        trajectory as replan_check is about to find it) and d2d_swept_crop behind the act launch (include/d2d_swept.h);
        `before_plan()`, a hook for tests, is called behind the mark with everything it read still in place"""
        noise = self.state.noise if self.cfg.noise_rows > 1 else None
        swept = self.swept is not None
        self._scan_snapshot()
        try:
            if self._plan.gaze != A.GAZE_NONE:
                self.backend.gaze_stage_live(self.cfg, self._st, self._plan)
            if noise is not None:                     # as rollout(): a single d2d_run_stages reads the block's first row
                self._st.noise = noise[self.cfg.noise_row0].data_ptr()
            if self.rvo:
                self._rvo_agents_live()
            self.backend.run_stages(self.cfg, self._st, (A.ST_PERCEIVE & ~A.ST_AGENTS if self.rvo else A.ST_PERCEIVE) | A.ST_SKIP_DONE)
            if swept:
                self.backend.swept_mark(self.cfg, self._st, self._plan, self._swept)
            if before_plan is not None:
                before_plan()
            self.backend.plan_stage_live(self.cfg, self._st, self._plan)
            self.backend.run_stages(self.cfg, self._st, A.ST_ACT | A.ST_SKIP_DONE)
            if swept:
                self.backend.swept_crop(self.cfg, self._st, self._swept)
            self._seen_update()
            self._scan_update()
            self._tracks_update()
            self._advance_noise(1)
        finally:
            if noise is not None:
                self._st.noise = noise.data_ptr()

    def policy_step(self):
        """One step of the reference's episode loop (experiment.py:69-70): a = policy.plan(info), then env.step(a), with the policy
        on the device.  Returns what step() returns.  Oxford's own maps (the time since a cell was observed) are not kept: under
        this planner they never reach an action; seen_obs=True keeps the same map as a channel of its own (include/d2d_seen.h)."""
        self._needs_step_gaze('policy_step()')
        if self.plugins is not None:       # the Primitive plugins: one step of run_episodes' loop (an env that is done stays as it is)
            if self.num_envs:
                self._plugins_step()
            return self._result()
        self.run_gaze()
        self.run_step()
        return self._result()

    def run_episodes(self, max_steps=None, check_every=16, live=None):
        """Every env plays its episode to the end (experiment.py:66-70) and stays as it ended.  Stops when every env is done or after
        `max_steps` (default ceil(max_flight_time / dt) + 1: freezing ends every episode by then); the host looks at the flags once
        per `check_every` steps and synchronises at no other time.  Returns the steps run.

        With planner='Jerk_Primitive' a step is d2d_gaze_act, the two launches of include/d2d_rvo_live.h under RVO,
        d2d_run_stages(PERCEIVE | SKIP_DONE), d2d_jerk_plan_live (include/d2d_jerk_live.h), d2d_run_stages(ACT | SKIP_DONE): every
        launch leaves finished envs alone, and a finished env is frozen in everything -- drone, counters, flags, dmap, gt, kf,
        active, the action, the Owl state, its agents and their velocities, plan_ok / wp_valid / wp, jerk_choice, jerk_stat and the
        tracker bookkeeping are those of the step that ended its episode, as in a one-env run of the same world.  (Of the two
        velocity buffers that swap every step, agent_vel is the velocity; agent_vel_out is the scratch half, into which a masked
        launch copies a finished env's velocity so that the swap keeps it.)

        `live` chooses the loop for this planner.  None: the masked launches where the backend has them (supports_jerk_live, under
        RVO also supports_rvo_live), else the loop below.  True: the masked launches, NotImplementedError where the backend lacks
        one.  False: d2d_jerk_plan and, under RVO, the two launches of include/d2d_rvo.h for every env, finished or not, launch for
        launch the loop of before the masked launches existed: drone, counters, flags, dmap, gt, kf, active, the action and the Owl
        state of a finished env are still frozen, and that is all a CSV row reads, but its plan_ok, wp, jerk_choice, jerk_stat and
        tracker bookkeeping keep being rewritten and under RVO its agents keep moving.  It is there for A/B measurement
        (tools/jerk_episodes_bench.py) and for a caller that depended on it.  The Primitive plugins take no `live`: their loop
        is masked throughout.

        With the Primitive plugins (planner='Primitive', under either motion profile) a step is d2d_gaze_stage_live, under RVO the two
        launches of include/d2d_rvo_live.h, d2d_run_stages(PERCEIVE | SKIP_DONE), d2d_plan_stage_live, d2d_run_stages(ACT | SKIP_DONE),
        and a finished env is frozen in everything: the fields above, its agents and their velocities, plan_ok / wp_valid / wp and
        its plugin state (trajectory, header, boxes, seen_step, the Owl scores and held decision, the tracker bookkeeping).  reset()
        with a mask between two calls starts a fresh episode, policy and trajectory for the envs of the mask alone."""
        self._needs_step_gaze('run_episodes()')
        n = int(np.ceil(self.params.max_flight_time / self.params.dt)) + 1 if max_steps is None else int(max_steps)
        every = max(1, int(check_every))
        if self.plugins is not None:
            t = 0
            while t < n and self.num_envs:
                self._plugins_step()
                t += 1
                if t % every == 0 and t < n and bool(self.state.flags[:, A.F_DONE].all()):
                    break
            return t
        live = self._jerk_live(live)
        t = 0
        while t < n and self.num_envs:
            self._jerk_step(live)
            t += 1
            if t % every == 0 and t < n and bool(self.state.flags[:, A.F_DONE].all()):
                break
        return t

    def _jerk_step(self, live):
        """One step of the episode loop with planner='Jerk_Primitive' (run_episodes, stream_episodes): d2d_gaze_act, under RVO the two
        RVO launches, d2d_run_stages(PERCEIVE | SKIP_DONE) with this step's row of the noise, the plan, d2d_run_stages(ACT |
        SKIP_DONE).  `live`: the plan and RVO launches that leave finished envs alone (include/d2d_jerk_live.h, d2d_rvo_live.h),
        else the unmasked ones"""
        noise = self.state.noise if self.cfg.noise_rows > 1 else None
        self._scan_snapshot()
        try:
            self.run_gaze()
            if noise is not None:                     # as rollout(): a single d2d_run_stages reads the block's first row
                self._st.noise = noise[self.cfg.noise_row0].data_ptr()
            if self.rvo:
                self._rvo_agents_live() if live else self._rvo_agents()
            self.backend.run_stages(self.cfg, self._st, (A.ST_PERCEIVE & ~A.ST_AGENTS if self.rvo else A.ST_PERCEIVE) | A.ST_SKIP_DONE)
            if live:
                self.backend.jerk_plan_live(self._jerk_call, self.state.flags)
            else:
                self.run_jerk_plan()
            self.backend.run_stages(self.cfg, self._st, A.ST_ACT | A.ST_SKIP_DONE)
            self._seen_update()
            self._scan_update()
            self._tracks_update()
            self._advance_noise(1)
        finally:
            if noise is not None:
                self._st.noise = noise.data_ptr()

    def run_jerk_plan(self):
        """d2d_jerk_plan for every env: plan_ok / wp_valid / wp of this step, from what d2d_perceive left"""
        if self.num_envs:
            self.backend.jerk_plan(self._jerk_call)

    @property
    def jerk_choice(self):
        """[B] int32: the heading index (theta / 5) the latest plan chose, -1 where it failed"""
        return self.jerk.t['choice']

    @property
    def jerk_stat(self):
        """[B] int32: include/d2d_jerk.h D2D_JERK_STAT_*"""
        return self.jerk.t['stat']

    def run_perceive(self, stages=A.ST_PERCEIVE):
        """d2d_perceive, or the stages of it named; the agents stage is the RVO launches under RVO"""
        if self.rvo and stages & A.ST_AGENTS:
            self._rvo_agents()
            stages &= ~A.ST_AGENTS
        if stages == A.ST_PERCEIVE:
            self.backend.perceive(self.cfg, self._st)
        elif stages:
            self.backend.run_stages(self.cfg, self._st, stages)

    def _set_action(self, actions):
        a = torch.as_tensor(actions, dtype=torch.float64)
        self.state.action.copy_(a.reshape(-1).expand(self.num_envs) if a.numel() == 1 else a.reshape(self.num_envs),
                                non_blocking=True)

    def set_plan(self, plan_ok, wp_valid, wp):
        """External planner result for this step (traj_planner.py Planner.plan + trajectory head)."""
        self.state.plan_ok.copy_(torch.as_tensor(plan_ok, dtype=torch.uint8).reshape(self.num_envs))
        self.state.wp_valid.copy_(torch.as_tensor(wp_valid, dtype=torch.uint8).reshape(self.num_envs))
        self.state.wp.copy_(torch.as_tensor(wp, dtype=torch.float64).reshape(self.num_envs, 6))

    def set_noise(self, noise):
        """Standard-normal draws for the measurements (utils.py:605) in place of the ones the device draws from the env's own
        stream; required when var_cam != 0 on a backend without that stage (the reference takes them from np.random in agent
        order).  [B, N, 2]: the draws of the next step (every step of a multi-step call would reuse them); [T, B, N, 2]: a run of multi-step calls (rollout() / closed_loop()) draws row after row, step t of the run from
        row t % T, as the reference draws fresh normals every step -- also when the run is cut into several calls
        (d2d_cfg.noise_row0 is advanced by the steps of every call; set_noise() starts again at row 0)."""
        n = torch.as_tensor(noise, dtype=torch.float64)
        rows = n.shape[0] if n.dim() == 4 else 1
        n = n.reshape(rows, self.num_envs, self.cfg.N, 2).to(self.device).contiguous()
        self.state.noise = n
        self._own_noise = True
        self._st.noise = n.data_ptr()
        self.cfg.noise_rows = rows
        self.cfg.noise_row0 = 0

    def _advance_noise(self, nsteps):
        if self.cfg.noise_rows > 1:
            self.cfg.noise_row0 = (self.cfg.noise_row0 + int(nsteps)) % self.cfg.noise_rows

    def step(self, actions):
        """One fused Drone2DEnv2.step for every env.  Returns (obs, reward, done, info) of tensors."""
        self._set_action(actions)
        self.run_step()
        return self._result()

    def perceive(self):
        """First half of step() (lines 153-187); a host planner plugin runs after this (the device Jerk_Primitive planner runs
        here, as the last part of this half).  With scan_obs the rays are ready behind this half: the pose has not moved yet."""
        self._scan_snapshot()
        self.run_perceive()
        if self.jerk is not None:
            self.run_jerk_plan()
        self._scan_update()

    def act(self, actions):
        """Second half of step() (lines 198-255)."""
        self._set_action(actions)
        self.backend.act(self.cfg, self._st)
        self._seen_update()
        self._tracks_update()
        return self._result()

    def rollout(self, actions, pin=None, collisions=False, streams=1):
        """`actions`: [T, B] gaze actions; T fused steps queued by one call (survivability-style sweeps,
        glob_survivability_calculator.py:31-37).  `pin`: [B, 2] drone position forced before each step.
        `streams` > 1 cuts the batch into that many independent sub-batches whose T-step chains run on their own
        HIP streams (envs are independent, so the chains need no ordering between them; on MI355X two chains of
        2048 envs finish ~16 % sooner than one of 4096 because kernel tails and launch gaps overlap)."""
        if self.seen is not None:
            raise NotImplementedError('rollout(): seen_obs=True does not run inside a fused rollout (its steps would go unseen by the '
                                      'time-since-observed map, whose launch of include/d2d_seen.h follows every single step); step '
                                      'the env with step() / action_stream() / policy_step() / run_episodes()')
        if self.scan is not None:
            raise NotImplementedError('rollout(): scan_obs=True does not run inside a fused rollout (the rays of its steps would be gone: '
                                      'the launch of include/d2d_scan.h follows every single step, from the pose in front of it); step '
                                      'the env with step() / action_stream() / policy_step() / run_episodes()')
        if self.tracks is not None:
            raise NotImplementedError('rollout(): tracks_obs=True does not run inside a fused rollout (its steps would go unseen by the '
                                      'tracker-forecast map, whose launch of include/d2d_tracks.h follows every single step); step '
                                      'the env with step() / action_stream() / policy_step() / run_episodes()')
        actions = torch.as_tensor(actions, dtype=torch.float64, device=self.device).contiguous()
        T = actions.shape[0]
        assert actions.shape == (T, self.num_envs)
        if pin is not None:
            pin = torch.as_tensor(pin, dtype=torch.float64, device=self.device).contiguous()
        coll = torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device) if collisions else None
        if self.rvo or self.jerk is not None:
            # a host loop of the RVO step (and of the Jerk_Primitive step, whose plan is a launch of another library) (`streams` is ignored): pin = a copy into the drone record before each step, collisions =
            # a copy of the flag after it, as d2d_rollout does them
            # With a [rows, B, N, 2] block of draws step t of the run takes row (row0 + t) % rows, as d2d_rollout does.  A single
            # d2d_run_stages reads the block's first row whatever noise_row0 says, so each step is handed its own row.
            noise = self.state.noise if self.cfg.noise_rows > 1 else None
            try:
                for t in range(T):
                    if pin is not None:
                        self.state.drone[:, A.D_X:A.D_Y + 1] = pin
                    self.state.action.copy_(actions[t])
                    if noise is not None:
                        self._st.noise = noise[self.cfg.noise_row0].data_ptr()
                    self.run_step()
                    self._advance_noise(1)
                    if collisions:
                        coll[t] = self.state.flags[:, A.F_COLLISION]
            finally:
                if noise is not None:
                    self._st.noise = noise.data_ptr()
            return coll
        S = max(1, min(int(streams), self.num_envs))
        if S == 1 or self.device.type != 'cuda' or (self.state.noise is not None and self.cfg.noise_rows > 1):
            self.backend.rollout(self.cfg, self._st, T, actions, pin, coll)
            self._advance_noise(T)
            return coll
        # sub-batch i owns envs [lo, hi): its own cfg (B = hi - lo) and state struct (every pointer offset by lo)
        import copy
        cur = torch.cuda.current_stream(self.device)
        bounds = [(self.num_envs * i) // S for i in range(S + 1)]
        subs = []
        for i in range(S):
            lo, hi = bounds[i], bounds[i + 1]
            if hi == lo:
                continue
            cfg = copy.copy(self.cfg)
            cfg.B = hi - lo
            st = A.State()
            for name in A.STATE_FIELDS:
                t = self.state.noise if name == 'noise' else self.state.t.get(name)
                base = getattr(self._st, name)
                stride = 0 if t is None else (t.stride(1) if name == 'noise' else t.stride(0))   # noise: [rows][B][N][2]
                setattr(st, name, None if (t is None or not base) else base + lo * stride * t.element_size())
            # the step-t row of a sub-batch is not contiguous in [T, B]: give each sub-batch its own copies (made on the
            # current stream, like everything the caller queued before this call)
            a_i = actions[:, lo:hi].contiguous()
            p_i = None if pin is None else pin[lo:hi].contiguous()
            # every step writes its whole row of collision flags: no fill, so nothing on the current stream can land
            # after a side stream's first step
            c_i = torch.empty((T, hi - lo), dtype=torch.uint8, device=self.device) if collisions else None
            subs.append((lo, hi, cfg, st, a_i, p_i, c_i, torch.cuda.Stream(self.device)))
        # the side streams start after EVERYTHING queued so far on the current stream, the per-sub-batch copies included
        ready = torch.cuda.Event()
        ready.record(cur)
        for lo, hi, cfg, st, a_i, p_i, c_i, stream in subs:
            stream.wait_event(ready)
            with torch.cuda.stream(stream):
                self.backend.rollout(cfg, st, T, a_i, p_i, c_i)
            for t_ in (a_i, p_i, c_i):       # allocated on the current stream, consumed on `stream`
                if t_ is not None:
                    t_.record_stream(stream)
        for lo, hi, cfg, st, a_i, p_i, c_i, stream in subs:
            cur.wait_stream(stream)
            if collisions:
                coll[:, lo:hi] = c_i
        return coll

    def _result(self):
        s = self.state
        obs = {'local_map': s.obs_local.unsqueeze(1), 'swep_map': s.obs_local.unsqueeze(1),   # drone_v2.py:251-255
               'yaw_angle': s.obs_yaw.unsqueeze(1)}
        if self.swept is not None:             # training_v3.py:206-213: the crop of what replan_check returned
            obs['swep_map'] = self.swept['obs'].unsqueeze(1)
        if self.seen is not None:              # the crop of Oxford.last_time_observed_map for the pose the env is in
            obs['age_map'] = self.seen['obs'].unsqueeze(1)
        if self.scan is not None:              # one range and one outcome per ray of the latest step's raycast
            obs['scan'] = self.scan['obs']
        if self.tracks is not None:            # the window of the tracker-forecast map, as float32
            obs['track_map'] = self.tracks['obs'].unsqueeze(1)
        done = s.flags[:, A.F_DONE].bool()
        info = {'collision_flag': s.flags[:, A.F_COLLISION], 'dead_lock_flag': s.flags[:, A.F_DEADLOCK],
                'freezing_flag': s.flags[:, A.F_FREEZING], 'state_machine': s.counters[:, A.C_SM],
                'flight_time': s.counters[:, A.C_STEPS].double() * self.cfg.dt,
                'tracked_agent': s.counters[:, A.C_TRACKED], 'newly_tracked': s.newly, 'hit': s.hit}
        return obs, self.reward, done, info

    # ------------------------------------------------------------------ a stream of seeded episodes over the resident slots
    def _needs_stream(self, num_episodes, episodes=None, external=False):
        """The refusals of stream_episodes(), in its order; `external`: of action_stream(), which differs in the gaze clause alone (the
        caller's actions in place of a policy the device evaluates) and keeps every other text"""
        backend_for(self.backend, None, 'supports_device_worlds', 'has no device world construction, which stream_episodes() rebuilds '
                    'a finished slot with: run the episodes as batches (runner.ExperimentBatch / SteppedExperimentBatch)')
        backend_for(self.backend, None, 'supports_episode_stream', 'has no launches that refill a finished slot '
                    '(include/d2d_worlds_stream.h): run the episodes as batches (runner.ExperimentBatch / SteppedExperimentBatch)')
        if self._streamed:
            raise RuntimeError('stream_episodes(): this env has streamed episodes already, so its slots hold the last worlds that '
                               'passed through them, not map ids map_id + 0 ..; build a new VecDrone2DEnv / EpisodeStream for another run')
        if episodes is not None:
            backend_for(self.backend, None, 'supports_episode_table', 'has no assignment from an episode table '
                        '(include/d2d_worlds_table.h): run the table as batches of host-built worlds (build_worlds_of)')
            if num_episodes is not None and int(num_episodes) != len(episodes):
                raise ValueError(f'stream_episodes(): num_episodes {num_episodes} with a table of {len(episodes)} episodes; leave it out')
        if (self._world_inp if episodes is None else self._table_inp) is None:
            raise NotImplementedError("stream_episodes(): the worlds of this env were built on the host or handed over; a finished slot "
                                      "is rebuilt on the device from its map id, so build the env with worlds='device'")
        if self._own_noise:
            raise NotImplementedError('stream_episodes(): set_noise() rows belong to the envs they were drawn for, not to the episodes '
                                      'that pass through a slot; leave the draws to the device (var_cam != 0 on a backend with '
                                      'supports_device_noise) or run the episodes as batches')
        if self.cfg.sigma != 0.0 and not self.device_noise:
            raise NotImplementedError('stream_episodes(): var_cam != 0 needs a backend that draws the measurement noise on the device '
                                      '(supports_device_noise); run the episodes as batches with set_noise()')
        if external:
            if self.device_gaze is not None or not ((self.plugins is not None and self.plugins.planner == A.PLAN_PRIMITIVE) or self.jerk is not None):
                raise RuntimeError("action_stream() needs device_plugins=True, planner='Primitive' or 'Jerk_Primitive' and gaze='external' "
                                   '(the caller supplies the action of every step); stream_episodes() plays the episodes of a gaze '
                                   'policy the device evaluates')
            backend_for(self.backend, None, 'supports_action_stream', 'has no restore and count launches for a stream the caller steps '
                        '(include/d2d_worlds_turn.h): step the env yourself with step() and reset(mask)')
            if self.plugins is not None and self.rvo:
                for flag, header in (('supports_stepped_plugins', 'd2d_stepped.h'), ('supports_rvo_live', 'd2d_rvo_live.h')):
                    backend_for(self.backend, None, flag, f'has no launches that leave finished envs alone (include/{header}): '
                                'action_stream() with the Primitive plugins under RVO runs on the HIP backend')
        elif self.device_gaze is None or (self.plugins is None and self.jerk is None):
            raise RuntimeError('stream_episodes() needs device_plugins=True and a gaze policy the device evaluates '
                               "(not gaze='external'); step the env yourself for anything else")
        elif self.plugins is not None and self.rvo:
            self._needs_step_gaze('stream_episodes()')
        if self.plugins is not None and self.swept is not None:    # the per-stage path under CVM too (_episode_steps)
            backend_for(self.backend, None, 'supports_stepped_plugins', 'has no gaze and plan stages that leave finished envs alone '
                        '(include/d2d_stepped.h): a stream with swept_obs=True runs one launch per stage')
        if self.jerk is not None and not self._jerk_live(None):
            self._jerk_live(True)              # raises, naming the launch that is missing
        M = int(num_episodes) if episodes is None else len(episodes)
        m0 = self.params.map_id + self.env_offset
        if M < 0 or M > A.STREAM_MAX_EPISODES:
            raise ValueError(f'stream_episodes(): {M} episodes: 0 <= num_episodes <= {A.STREAM_MAX_EPISODES}')
        if episodes is None and m0 + M > 2 ** 32:
            raise ValueError(f'stream_episodes(): map_id {m0} + {M} episodes passes 2**32: numpy seeds with 0 <= map_id < 2**32 only; '
                             'split the run into streams that end below it')
        if self.num_envs and M and bool(self.state.counters[:, A.C_STEPS].ne(0).any() | self.state.flags.ne(0).any()):
            # (one host read before the first step: the first min(B, M) episodes are the envs as constructed)
            raise RuntimeError('stream_episodes(): this env has been stepped, and the first episodes of a stream are the envs as '
                               'constructed; reset() it, or build a new VecDrone2DEnv / EpisodeStream')
        return M, (m0 if episodes is None else self._episode_table(episodes))

    # Params fields a table may vary from row to row: what d2d_worlds_build reads per env (d2d_world_spec.map_id, env_par, env_tgt)
    TABLE_PER_EPISODE = ('map_id', 'init_position', 'target_list', 'agent_radius', 'agent_max_speed')

    def episode_params(self, episodes):
        """table_params over the env's own Params"""
        return table_params(self.params, episodes)

    def _episode_table(self, episodes):
        """The table of stream_episodes(episodes=...) as the host arrays d2d_stream_assign_table reads (map_id [M] uint32, env_par
        [M, 8], env_tgt [M, T, 2]), or the ValueError that names the field and the row: a table varies what the world build reads per
        env -- map_id, init_position, target_list, and the agent radius and speed where the derived d2d_cfg stays equal -- and nothing
        the batch shares.  The planner and gaze tables read, of the fields a row may vary, agent_radius alone, which the Kalman
        archive bounds of d2d_cfg pin."""
        import ctypes
        p0, B = self.params, self.num_envs
        plist = self.episode_params(episodes)
        cfg_fields = [n for n, _ in A.Cfg._fields_]
        seen = {}
        for i, p in enumerate(plist):
            m = p.map_id
            if not (isinstance(m, (int, np.integer)) and 0 <= int(m) < 2 ** 32):
                raise ValueError(f'stream_episodes(): episode {i}: map_id {m!r}: numpy seeds with 0 <= map_id < 2**32 only')
            for name in sorted(set(vars(p0)) | set(vars(p))):
                if name in self.TABLE_PER_EPISODE:
                    continue
                a, b = getattr(p0, name, None), getattr(p, name, None)
                if (list(a) if isinstance(a, (list, tuple)) else a) != (list(b) if isinstance(b, (list, tuple)) else b):
                    raise ValueError(f'stream_episodes(): episode {i}: {name} = {b!r}, the stream has {a!r}: {name} is per stream '
                                     '(the batch shares its map, agent count, planner, gaze, motion profile and tables); a table '
                                     'varies ' + ', '.join(self.TABLE_PER_EPISODE))
            if max(len(p.target_list), 1) != self.cfg.T:
                raise ValueError(f'stream_episodes(): episode {i}: target_list has {len(p.target_list)} targets, the stream has '
                                 f'{self.cfg.T}: the number of targets is per stream')
            key = (p.agent_radius, p.agent_max_speed)
            if key not in seen:
                c = host_init.derive_cfg(p, B=B, N=self.cfg.N, T=self.cfg.T, planner_mode=self.planner_mode,
                                         kf_enabled=bool(self.cfg.kf_enabled), grid_tile=self.cfg.grid_tile)
                seen[key] = next((n for n in cfg_fields if n not in ('noise_rows', 'noise_row0') and getattr(c, n) != getattr(self.cfg, n)),
                                 None)
            if seen[key] is not None:
                n = seen[key]
                raise ValueError(f'stream_episodes(): episode {i}: agent_radius = {p.agent_radius!r} (the stream has {p0.agent_radius!r}) '
                                 f'moves d2d_cfg.{n}: the derived cfg is per stream')
            if float(p.agent_radius) != float(p0.agent_radius):
                raise ValueError(f'stream_episodes(): episode {i}: agent_radius = {p.agent_radius!r} (the stream has {p0.agent_radius!r}): '
                                 'the planner and gaze tables hold it, and they are per stream')
        if not plist:
            T = self.cfg.T
            return dict(map_id=np.zeros(0, np.uint32), env_par=np.zeros((0, A.WORLDS_ENV_F)), env_tgt=np.zeros((0, T, 2)), map_ids=[])
        tab = world_inputs(plist, redraw=self.redraw_agents)
        inp = self._table_inp
        if tab['N'] != self.cfg.N or tab['P'] != inp['P']:
            raise ValueError('stream_episodes(): episode 0: the table\'s static map gives another agent count than the env has')
        for i in range(min(B, len(plist))):
            for name in ('map_id', 'env_par', 'env_tgt'):
                if not np.array_equal(tab[name][i], inp[name][i]):
                    raise ValueError(f'stream_episodes(): episode {i}: {name} {tab[name][i].tolist()} is not that of env {i} as '
                                     f'constructed ({inp[name][i].tolist()}): the first min(num_envs, episodes) rows are the envs as '
                                     'constructed (runner.EpisodeStream(params, episodes=...) builds them so)')
        return {k: tab[k] for k in ('map_id', 'env_par', 'env_tgt', 'map_ids')}

    def _episode_steps(self, n):
        """`n` steps of the env's own episode loop, finished envs left alone: closed_loop(freeze_done=True) where closed_loop() runs,
        the step sequences of run_episodes() elsewhere -- and with swept_obs, whose map exists only between two stages of a step.
        With seen_obs, whose launch follows every single step, `n` times the path taken for n = 1"""
        if self.plugins is not None and not self.rvo and self.swept is None:
            if self.seen is None and self.scan is None and self.tracks is None:
                self.closed_loop(n, freeze_done=True)
                return
            for _ in range(n):             # the persistent launch, one step at a time
                self._scan_snapshot()
                self._closed_loop_steps(1, A.DONE_FREEZE)
                self._seen_update()
                self._scan_update()
                self._tracks_update()
        elif self.plugins is not None:
            for _ in range(n):
                self._plugins_step()
        else:
            for _ in range(n):
                self._jerk_step(True)

    def _refill_rest(self, refill):
        """Everything outside the world of the slots in `refill` ([B] uint8) as a fresh env has it: the masked resets of the plugin,
        Jerk_Primitive and gaze state (which read the tracker radii the build just wrote), and masked fills for the per-step
        outputs.  The flags were written by the build.  No host read"""
        s, m = self.state, refill.bool()
        for name in ('plan_ok', 'wp_valid', 'wp', 'hit', 'newly', 'obs_local', 'obs_yaw', 'rng_draws'):
            t = s.t.get(name)
            if t is not None and t.numel():
                t.masked_fill_(m.view((-1,) + (1,) * (t.dim() - 1)), 0)
        s.action.masked_fill_(m, 1.0 if self.device_gaze == 'Rotating' else 0.0)
        if self.rvo:                           # state.init_rvo: zero for the seeded agents, the preferred velocity for the static map's
            k = min(int(self.params.agent_number), self.cfg.N)
            vel = s.agent_vel
            vel[:, :, :k].masked_fill_(m[:, None, None], 0)
            vel[:, :, k:] = torch.where(m[:, None, None], s.agents[:, A.A_VX:A.A_VY + 1, k:], vel[:, :, k:])
        if self.plugins is not None:
            self.plugins.t['plan_stat'].masked_fill_(m[:, None], 0)
        # per-slot storage that no reset covers, zero in a fresh env: the trajectory and its boxes (dead beyond the header, which
        # d2d_plan_reset clears), the search's nodes and hash, the scratch half of the velocity swap.  d2d_stream_clear touches the
        # refilled slots alone, so the cost follows the slots rebuilt and not the batch
        for t in ([self.plugins.t[k] for k in ('traj', 'traj_box', 'nodes', 'hash')] if self.plugins is not None else []) + \
                ([s.agent_vel_out] if self.rvo else []):
            self.backend.stream_clear(t, refill)
        if self.jerk is not None:
            for name in ('choice', 'stat'):
                self.jerk.t[name].masked_fill_(m, 0)
        self._swept_zero(refill)
        self.reset_plugins(refill)
        self._seen_zero(refill)
        self._scan_zero(refill)
        self._tracks_update()              # (a refilled slot's counter jumped back: its window comes out zero)

    def stream_episodes(self, num_episodes=None, refill_every=64, max_attempts=None, trace=None, episodes=None, capture=None):
        """Episodes map_id + 0 .. map_id + num_episodes - 1 over the env's `num_envs` slots: a slot whose episode has ended is
        handed the next map id, its world is rebuilt in place on the device and everything that hangs on it is put back, so the
        slots stay full while the queue lasts and memory is bounded by the slots, not the episodes.  Returns the records
        [num_episodes, 8] int32 (include/d2d_worlds_stream.h D2D_STREAM_R_*; runner.EpisodeStream makes CSV rows of them).

        The first min(num_envs, num_episodes) episodes are the envs as constructed.  Every `refill_every` steps of the env's own
        episode loop (closed_loop(refill_every, freeze_done=True) where closed_loop() runs, the step sequences of run_episodes()
        elsewhere) come d2d_stream_harvest, d2d_stream_assign, d2d_worlds_build_masked and the masked resets; the 8 bytes of
        `finished` read back after the assignment are the loop's only synchronisation, and where they have not moved nothing was
        harvested and the build and the resets, which would all be no-ops, are not queued.  An episode depends on nothing but its
        world, so its record does not depend on `refill_every` or on the slot that played it.

        A world that cannot be placed within `max_attempts` (default: the constructor's) ends at once with column 0 of its record
        == STREAM_BUILD_FAILED.  `trace`: a list that receives (steps so far, slots live) per refill, for measurement (one more
        host read each).  The env has then played other worlds than its snapshot: reset() refuses afterwards.

        `episodes`: a table in place of consecutive map ids -- a list of Params, or of (map_id, init_position, target_list) triples
        over the env's own Params; episode k is the world of row k (include/d2d_worlds_table.h: the slot that receives it copies the
        row's map id, env_par and env_tgt, and the same masked build reads them).  This is a cell of the reference's validation
        study: 5 maps x 72 (start, target) pairs (runner.ValidationStudy).  A row varies map_id, init_position and target_list
        freely, and the agent radius and speed only where the derived d2d_cfg stays equal (the Kalman archive bounds take
        agent_radius); everything else is per stream, and a row that differs is refused with a ValueError that names the field and
        the row.  The first min(num_envs, len(episodes)) rows must be the envs as constructed, which runner.EpisodeStream(params,
        episodes=...) sees to.  With `redraw_agents` every row's world is redrawn.

        `capture`: a capture.Capture of this env -- in front of every harvest the finished slots of its kinds are drawn into its
        gallery on the device (include/d2d_capture.h), three more launches a refill and no host read."""
        for _ in self.stream_rounds(num_episodes, refill_every, max_attempts, trace, episodes, capture):
            pass
        return self.stream_rows

    def _stream_arrays(self, M, table, max_attempts=None):
        """What a stream of M > 0 episodes over the B > 0 slots keeps on the device (stream_rounds, action_stream.ActionStream): the
        spec's arrays `up`, the table's rows `ep` (or None), the d2d_world_spec of the masked build, slot_episode, the refill bytes and
        counts = (cursor, finished).  Retires the surplus slots and marks the env as streamed"""
        B, dev, s = self.num_envs, self.device, self.state
        inp = dict(self._world_inp if table is None else self._table_inp)
        if max_attempts is not None:
            inp['max_attempts'] = int(max_attempts)
        up = {n: torch.from_numpy(inp[n]).to(dev) for n in ('unit', 'cells', 'env_par', 'env_tgt')}
        up['map_id'] = torch.from_numpy(inp['map_id'].view(np.int32).copy()).to(dev)
        ep = None
        if table is not None:                  # the rows a slot copies when it is handed an episode (the launches only read them)
            ep = (torch.from_numpy(table['map_id'].view(np.int32).copy()).to(dev), torch.from_numpy(table['env_par']).to(dev),
                  torch.from_numpy(table['env_tgt']).to(dev))
        up['status'] = torch.zeros(B, dtype=torch.int32, device=dev)
        N, P = self.cfg.N, inp['P']
        radius0 = self.plugins.trk_radius0 if self.plugins is not None else self.jerk.trk_radius0     # [B, max(N, 1)]: the output's shape for N > 0
        up['tracker_radius'] = radius0
        up['obstacles'] = s.pillars if 'pillars' in s.t and tuple(s.pillars.shape) == (B, P, 3) else torch.zeros((B, P, 3), dtype=torch.int32, device=dev)
        spec = world_spec(inp, self.cfg.grid_tile, lambda n: up[n].data_ptr() if up[n].numel() else s._dummy.data_ptr())
        slot_episode = torch.arange(B, dtype=torch.int32, device=dev)
        refill = torch.zeros(B, dtype=torch.uint8, device=dev)
        counts = torch.tensor([min(B, M), 0], dtype=torch.int64, device=dev)
        if M < B:                              # the surplus slots are retired before the first step
            slot_episode[M:] = -1
            s.flags[M:, A.F_DONE] = 1
        self._streamed = True
        self._stream_keep = (up, slot_episode, refill, counts, ep)   # (the launches are asynchronous: the arrays outlive them)
        return up, ep, spec, slot_episode, refill, counts

    def stream_rounds(self, num_episodes=None, refill_every=64, max_attempts=None, trace=None, episodes=None, capture=None):
        """stream_episodes() as a generator that hands control back after every refill that rebuilt a slot: yields (episodes finished,
        the refill bytes [B] uint8 of the round); the records so far are `stream_rows`.  For callers that look at the slots in
        between (the tests do)."""
        M, m0 = self._needs_stream(num_episodes, episodes)        # m0: the first map id, or the table's arrays
        table = None if episodes is None else m0
        B, dev, s = self.num_envs, self.device, self.state
        every = max(1, int(refill_every))
        self.stream_rows = rows = torch.full((M, A.STREAM_ROW_F), -1, dtype=torch.int32, device=dev)
        self.steps_streamed = 0
        if M == 0 or B == 0:
            return
        owner = object()
        if capture is not None:
            capture.attach(self, owner)
        try:
            yield from self._stream_loop(M, m0, table, every, max_attempts, trace, capture, rows)
        finally:
            if capture is not None:
                capture.detach(owner)
        self.sync()

    def _stream_loop(self, M, m0, table, every, max_attempts, trace, capture, rows):
        """the rounds of stream_rounds() for M > 0 episodes over B > 0 slots"""
        B, s = self.num_envs, self.state
        up, ep, spec, slot_episode, refill, counts = self._stream_arrays(M, table, max_attempts)
        finished, guard = 0, (-(-M // B) + 1) * (int(np.ceil(self.params.max_flight_time / self.params.dt)) + 1 + every)
        while finished < M:
            if self.steps_streamed > guard:
                raise RuntimeError(f'stream_episodes(): {finished} of {M} episodes after {self.steps_streamed} steps: an episode did not end')
            self._episode_steps(every)
            self.steps_streamed += every
            if capture is not None:            # the slots the harvest is about to record, drawn as they ended
                capture.queue(slot_episode)
            self.backend.stream_harvest(self.cfg, self._st, slot_episode, rows)
            if table is None:
                self.backend.stream_assign(s.flags, M, m0, slot_episode, up['map_id'], refill, counts)
            else:
                self.backend.stream_assign_table(s.flags, ep[0], ep[1], ep[2], slot_episode, up['map_id'], up['env_par'], up['env_tgt'],
                                                 refill, counts)
            now = int(counts[1])               # the only host read
            if trace is not None:
                trace.append((self.steps_streamed, int((s.flags[:, A.F_DONE] == 0).sum()) + int(refill.sum())))
            if now == finished:
                continue
            finished = now
            if finished >= M:                  # the queue is dry and every slot retired: nothing to rebuild
                break
            self.backend.build_worlds_masked(spec, self._st, refill)
            self._refill_rest(refill)
            yield finished, refill

    def action_stream(self, num_episodes=None, refill_every=4, max_attempts=None, episodes=None, capture=None):
        """A stream of seeded episodes over the env's slots that the caller steps with its own gaze actions (action_stream.ActionStream):
        `stream.step(actions)` takes [B] float64 on the device and returns (obs, terms, done, info), and a slot whose episode has ended
        is in the next seeded world at the caller's next step -- harvest, assignment, masked build, d2d_stream_restore
        (include/d2d_worlds_turn.h) and the masked resets are queued at the start of every `refill_every`-th call, and nothing is read
        back.  For an env built with device_plugins=True, planner='Primitive' or 'Jerk_Primitive', gaze='external' and
        worlds='device', under either motion profile; every other refusal is stream_episodes()'s, in its words.

        Episodes, `max_attempts` and `episodes` (a table) are stream_episodes()'s.  `num_episodes=None` without a table: as many as
        the records can number, STREAM_MAX_EPISODES clipped to the map ids below 2**32 -- `rows` is allocated for all of them
        (32 bytes an episode), so a learner that knows its budget passes it.

        `capture`: a capture.Capture of this env, filled by every turn and by close() in front of their harvest (three more launches
        each, queued unconditionally; step() still reads nothing)."""
        from .action_stream import ActionStream
        m0 = self.params.map_id + self.env_offset
        if num_episodes is None and episodes is None:
            num_episodes = max(0, min(A.STREAM_MAX_EPISODES, 2 ** 32 - m0))
        M, first = self._needs_stream(num_episodes, episodes, external=True)
        return ActionStream(self, M, first, None if episodes is None else first, refill_every, max_attempts, capture)

    def closed_loop(self, nsteps=1, auto_reset=False, freeze_done=False):
        """`nsteps` reference-style steps with the plugins on the device: a = Oxford.plan(info); perceive;
        Primitive.replan_check + plan; act (experiment.py:68-70).  `auto_reset`: an env whose episode ended restarts
        from its seeded world with fresh plugin state at its next step.  `freeze_done`: an env whose episode ended
        stays as it ended (one episode per env; `episode_stats()` then holds one CSV row per env)."""
        if self.jerk is not None:
            raise NotImplementedError("closed_loop(): planner 'Jerk_Primitive' does not run inside the persistent closed loop (its "
                                      'stage lives in libd2d_jerk.so); step the env with step() / perceive() + act(), or run '
                                      'episodes through runner.Experiment.  run_episodes() / runner.SteppedExperimentBatch play '
                                      'whole episodes of this planner as a batch')
        if self.plugins is None:
            raise RuntimeError('closed_loop() needs device_plugins=True')
        if self.rvo:
            raise NotImplementedError("closed_loop(): motion_profile 'RVO' does not run inside the persistent closed loop (its stage "
                                      'lives in libd2d_rvo.so); step the env with step() / perceive() + act(), or run episodes '
                                      'through runner.Experiment.  run_episodes() / runner.SteppedExperimentBatch play whole '
                                      'episodes under this profile as a batch')
        if self.swept is not None:
            raise NotImplementedError('closed_loop(): swept_obs=True does not run inside the persistent closed loop (the swept map '
                                      'exists only between the perceive and the plan stage of a step, and the launches of '
                                      'include/d2d_swept.h go between them); step the env with action_stream() / policy_step() / '
                                      'run_episodes(), which run one launch per stage')
        if self.seen is not None:
            raise NotImplementedError('closed_loop(): seen_obs=True does not run inside the persistent closed loop (its steps would go '
                                      'unseen by the time-since-observed map, whose launch of include/d2d_seen.h follows every single '
                                      'step); step the env with action_stream() / policy_step() / run_episodes()')
        if self.tracks is not None:
            raise NotImplementedError('closed_loop(): tracks_obs=True does not run inside the persistent closed loop (its steps would go '
                                      'unseen by the tracker-forecast map, whose launch of include/d2d_tracks.h follows every single '
                                      'step); step the env with action_stream() / policy_step() / run_episodes()')
        if self.scan is not None and (int(nsteps) > 1 or auto_reset):
            raise NotImplementedError('closed_loop(): scan_obs=True takes one step a call and no auto_reset (inside the persistent loop the '
                                      'rays of its steps would be gone: the launch of include/d2d_scan.h follows every single step, from '
                                      'the pose in front of it); step the env with action_stream() / policy_step() / run_episodes()')
        if auto_reset and self._streamed:
            raise RuntimeError('closed_loop(auto_reset=True): this env has streamed episodes (stream_episodes), so its slots hold other '
                               'worlds than the snapshot an auto reset restores; build a new VecDrone2DEnv for the map ids you want')
        mode = A.DONE_RESET if auto_reset else (A.DONE_FREEZE if freeze_done else A.DONE_CONTINUE)
        self._scan_snapshot()
        self._closed_loop_steps(nsteps, mode)
        self._scan_update()                # (a single step: more are refused above)
        return self._result()

    def _closed_loop_steps(self, nsteps, mode):
        """d2d_closed_loop for `nsteps` steps under `mode` (DONE_*), the refusals of closed_loop() behind it"""
        self.backend.closed_loop(self.cfg, self._st, self._plan, int(nsteps), mode, self._init_st if mode == A.DONE_RESET else None)
        self._advance_noise(nsteps)

    def reset_plugins(self, mask=None):
        if self.plugins is not None:
            if mask is not None:
                mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            self.backend.plan_reset(self.cfg, self._plan, mask, 1)
        if self.jerk is not None and self.num_envs and self.cfg.N:
            if mask is not None:
                mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            self.backend.jerk_reset(self.jerk.t['trk_radius'], self.jerk.t['trk_prev'], self.jerk.trk_radius0, mask, 1)
        if self.gaze_state is not None and self.gaze_state.owl_state is not None and self.num_envs:
            if mask is not None:
                mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            self.backend.gaze_reset(self.gaze_state.owl_state, mask, 1)

    def sync(self):
        self.backend.sync()

    # ------------------------------------------------------------------ the renderer (include/d2d_render.h, render.py)
    def render_list(self, slots=None, trajectories=None):
        """The display list of `slots` (None: all; an int32 / int64 tensor or a list, repeats and any order allowed): the draw calls
        of Drone2DEnv2.render behind the cell layer (envs/drone_v2.py:263-303), in its order and with its float64 numbers, as a dict
        of device tensors -- kind [S, cap] int32 (_abi.RK_*), rgb [S, cap, 3], npts, width [S, cap], geom [S, cap, 20] float64, count
        [S] and status [S] (RENDER_OVERFLOW: the list did not fit, count is 0).  For callers who draw vector graphics themselves.
        Scratch of the next call; nothing is read back and nothing of the env is written."""
        from . import render
        return render.lists(self, slots, trajectories)

    def render_frames(self, slots=None, downsample=1, out=None, trajectories=None):
        """[S, Hf, Wf, 3] uint8 on the device: the picture Drone2DEnv2.render draws, of every slot of `slots` as it stands (a finished
        slot: its terminal state), point-sampled at every `downsample`-th pixel of every `downsample`-th row (Hf = ceil(H_px / d),
        Wf = ceil(W_px / d)) and rasterised by the rules of include/d2d_render.h.  `out`: a contiguous uint8 tensor with at least S
        such rows to draw into; rows from S on are left alone.  `trajectories`: the stored trajectory's positions where a host planner
        holds them -- a list of S arrays [n, 2], or (traj [S, K, 2] float64, traj_len [S] int32); otherwise the device Primitive
        planner's, and none under NoMove and Jerk_Primitive.  Two launches, no host read, nothing of the env written."""
        from . import render
        return render.frames(self, slots, downsample, out, trajectories)

    # ------------------------------------------------------------------ slot forks (include/d2d_fork.h, fork.py)
    def fork_items(self, src_env=None):
        """[(name, dst tensor, src tensor)] of every per-slot tensor a slot's future depends on or a caller can read, `dst` this env's
        and `src` that of `src_env` (default: this env): all of state.t (the noise stream, the pillars and under RVO both halves of
        the velocity swap, by the names they stand for now), plugins.t but for the launch arguments, jerk.t, both trk_radius0, the
        gaze state and the dicts of the four observation channels.  What is not listed, and why, is fork.EXCLUDED; the reset
        snapshot (init_state) is not a holder: reset() refuses after a load.  A loop over `.cpu()` of it saves a batch to the host."""
        from . import fork
        return fork.items_of(self, self if src_env is None else src_env)

    def load_slots(self, src_env, src_of):
        """Slot e of this env becomes slot src_of[e] of `src_env`, in everything fork_items() lists, by one launch and without a
        host read (d2d_fork_slots).  `src_of`: [num_envs] int32 on the device; -1 leaves the slot alone.  Returns `status`
        [num_envs] uint8 on the device: FORK_LEFT 0, FORK_COPIED 1, FORK_REFUSED 2 (src_of[e] >= src_env.num_envs).

        The two envs are the same in everything but the number of slots -- every cfg field but B, planner, device_plugins, gaze,
        motion profile, observation channels, and so the names and rows of their items -- or the call raises a ValueError that names
        the field; sibling() builds such an env.  Neither has set_noise() rows installed, and this env has no open action_stream();
        the SOURCE may have one, it is only read: that is the what-if from a live stream (whatif.branch_terms).  Afterwards this env
        has played other worlds than its snapshot: reset() and closed_loop(auto_reset=True) refuse, as after a stream."""
        from . import fork
        return fork.load_slots(self, src_env, src_of, in_place=src_env is self)

    def fork(self, src_of):
        """load_slots(self, src_of): slot e becomes slot src_of[e] of this same env.  A slot may be read only if it is not written
        in the same launch: slot e with s = src_of[e] != e is copied only when src_of[s] < 0 or src_of[s] == s, and is refused
        otherwise (status 2, nothing of it written) -- so `src_of = [0, 0, 0, 0]` fans slot 0 out, and a permutation is refused slot
        by slot.  The rule reads src_of alone, so the result depends on no order; src_of[e] == e or < 0 leaves slot e alone."""
        return self.load_slots(self, src_of)

    def sibling(self, num_envs, backend=None):
        """A second env of `num_envs` slots built with the arguments this one was built with, the backend included (`backend`: another
        one, for backends that serve one env each): what load_slots() loads branches into.  Worlds that were handed over are handed
        on, repeated or cut to `num_envs`; the slots' first contents matter to nobody who loads them."""
        a = dict(self._ctor)
        w, n = a['worlds'], int(num_envs)
        if isinstance(w, DeviceWorlds):
            idx = torch.arange(n, device=w.state.device) % max(w.num_envs, 1)
            a['worlds'] = w.spread(idx if w.index is None else w.index.to(idx.device)[idx])
        elif isinstance(w, (list, tuple)):
            a['worlds'] = [w[i % len(w)] for i in range(n)] if w else w
        if backend is not None:
            a['backend'] = backend
        elif a['backend'] is None:
            a['backend'] = self.backend
        params = a.pop('params')
        return type(self)(params, n, **a)

    # ------------------------------------------------------------------ episode statistics (CSV row, experiment.py:73-103)
    def episode_stats(self):
        """Per-env int64 [B, 8]: steps, success, static collision, dynamic collision, freezing, dead lock,
        grid discovered, agents tracked."""
        s = self.state
        c = s.counters.long()
        f = s.flags.long()
        disc = (s.dmap != 0).flatten(1).sum(1)
        return torch.stack([c[:, A.C_STEPS], (c[:, A.C_SM] == A.SM_GOAL_REACHED).long(), (f[:, 0] == 1).long(),
                            (f[:, 0] == 2).long(), f[:, 2], f[:, 1], disc, c[:, A.C_BUF_N]], dim=1)
