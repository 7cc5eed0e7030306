"""Loader of the HIP library (csrc/libd2d_hip.so).  There is NO CPU fallback: if the library is missing
or its ABI does not match, importing the backend raises."""
import ctypes as C
import os

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('D2D_LIB') or os.path.join(_HERE, 'csrc', 'libd2d_hip.so')   # D2D_LIB: A/B builds
WORLDS_LIB_PATH = os.path.join(_HERE, 'csrc', 'worlds', 'libd2d_worlds.so')             # include/d2d_worlds.h
METRICS_LIB_PATH = os.path.join(_HERE, 'csrc', 'metrics', 'libd2d_metrics.so')          # include/d2d_metrics.h
RVO_LIB_PATH = os.path.join(_HERE, 'csrc', 'rvo', 'libd2d_rvo.so')                      # include/d2d_rvo.h
JERK_LIB_PATH = os.path.join(_HERE, 'csrc', 'jerk', 'libd2d_jerk.so')                   # include/d2d_jerk.h
GAZE_LIB_PATH = os.path.join(_HERE, 'csrc', 'gaze', 'libd2d_gaze.so')                   # include/d2d_gaze.h
SEEN_LIB_PATH = os.path.join(_HERE, 'csrc', 'seen', 'libd2d_seen.so')                   # include/d2d_seen.h
SCAN_LIB_PATH = os.path.join(_HERE, 'csrc', 'scan', 'libd2d_scan.so')                   # include/d2d_scan.h
TRACKS_LIB_PATH = os.path.join(_HERE, 'csrc', 'tracks', 'libd2d_tracks.so')             # include/d2d_tracks.h
FORK_LIB_PATH = os.path.join(_HERE, 'csrc', 'fork', 'libd2d_fork.so')                   # include/d2d_fork.h
RENDER_LIB_PATH = os.path.join(_HERE, 'csrc', 'render', 'libd2d_render.so')             # include/d2d_render.h


class D2DError(RuntimeError):
    pass


def launch_shape(cfg, plan=None, fn=None):
    """(waves per workgroup, LDS bytes per workgroup, workgroups per CU by LDS, specialised kernels?) -- d2d_launch_shape;
    needs no GPU."""
    if fn is None:
        fn = load_library()[1]
    out = (C.c_int32 * 4)()
    _check(fn['launch_shape'](C.byref(cfg), None if plan is None else C.byref(plan), C.byref(out)), fn, 'd2d')
    return tuple(out)


# file name -> (binder, version entry point, the expected version's name in _abi (read at the call), noun of the mismatch text,
# build script under gym-drone2d-activeperception_amd/csrc/)
_LIBRARIES = {
    'libd2d_hip.so': (A.bind, 'abi_version', 'D2D_ABI_VERSION', 'ABI', 'build.sh'),
    'libd2d_worlds.so': (A.bind_worlds, 'version', 'D2D_WORLDS_VERSION', 'version', 'worlds/build.sh'),
    'libd2d_metrics.so': (A.bind_metrics, 'version', 'D2D_METRICS_VERSION', 'version', 'metrics/build.sh'),
    'libd2d_rvo.so': (A.bind_rvo, 'version', 'D2D_RVO_VERSION', 'version', 'rvo/build.sh'),
    'libd2d_jerk.so': (A.bind_jerk, 'version', 'D2D_JERK_VERSION', 'version', 'jerk/build.sh'),
    'libd2d_gaze.so': (A.bind_gaze, 'version', 'D2D_GAZE_VERSION', 'version', 'gaze/build.sh'),
    'libd2d_seen.so': (A.bind_seen, 'version', 'D2D_SEEN_VERSION', 'version', 'seen/build.sh'),
    'libd2d_scan.so': (A.bind_scan, 'version', 'D2D_SCAN_VERSION', 'version', 'scan/build.sh'),
    'libd2d_tracks.so': (A.bind_tracks, 'version', 'D2D_TRACKS_VERSION', 'version', 'tracks/build.sh'),
    'libd2d_fork.so': (A.bind_fork, 'version', 'D2D_FORK_VERSION', 'version', 'fork/build.sh'),
    'libd2d_render.so': (A.bind_render, 'version', 'D2D_RENDER_VERSION', 'version', 'render/build.sh'),
}


def _load(name, path):
    binder, version_fn, version, noun, script = _LIBRARIES[name]
    # torch first: its bundled HIP runtime has to be the one the library binds to.  Loaded the other way round the process ends up
    # with two runtimes and every launch fails with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    if not os.path.isfile(path):
        raise D2DError(f'{path} not found: build it with gym-drone2d-activeperception_amd/csrc/{script} '
                       '(or __graft_entry__.build()); there is no CPU fallback')
    lib = C.CDLL(path)
    fn = binder(lib)
    v, want = fn[version_fn](), getattr(A, version)
    if v != want:
        raise D2DError(f'{name} {noun} {v} != expected {want}: rebuild')
    return lib, fn


def load_library(path=LIB_PATH):
    return _load('libd2d_hip.so', path)


def load_worlds_library(path=WORLDS_LIB_PATH):
    """The world construction's own library (include/d2d_worlds.h)."""
    return _load('libd2d_worlds.so', path)


def load_metrics_library(path=METRICS_LIB_PATH):
    """The difficulty metrics' own library (include/d2d_metrics.h)."""
    return _load('libd2d_metrics.so', path)


def load_rvo_library(path=RVO_LIB_PATH):
    """The RVO motion profile's own library (include/d2d_rvo.h)."""
    return _load('libd2d_rvo.so', path)


def load_jerk_library(path=JERK_LIB_PATH):
    """The Jerk_Primitive planner's own library (include/d2d_jerk.h)."""
    return _load('libd2d_jerk.so', path)


def load_gaze_library(path=GAZE_LIB_PATH):
    """The step path's gaze decision, a library of its own (include/d2d_gaze.h)."""
    return _load('libd2d_gaze.so', path)


def load_seen_library(path=SEEN_LIB_PATH):
    """The time-since-observed map as an observation channel, a library of its own (include/d2d_seen.h)."""
    return _load('libd2d_seen.so', path)


def load_scan_library(path=SCAN_LIB_PATH):
    """The per-ray scan of the raycast, a library of its own (include/d2d_scan.h)."""
    return _load('libd2d_scan.so', path)


def load_tracks_library(path=TRACKS_LIB_PATH):
    """The tracker-forecast map as an observation channel, a library of its own (include/d2d_tracks.h)."""
    return _load('libd2d_tracks.so', path)


def load_fork_library(path=FORK_LIB_PATH):
    """The slot fork, a library of its own (include/d2d_fork.h)."""
    return _load('libd2d_fork.so', path)


def load_render_library(path=RENDER_LIB_PATH):
    """The renderer, a library of its own (include/d2d_render.h)."""
    return _load('libd2d_render.so', path)


def _check(rc, fn, label):
    if rc != 0:
        raise D2DError(f'{label} error {rc}: {fn["last_error"]().decode()}')


def backend_for(backend, device, flag=None, lacks=None):
    """`backend`, or the HIP backend of `device` where it is None (which raises if a library or the GPU is missing).  With `flag`
    (a supports_* attribute) a backend without it is refused: NotImplementedError('<its name> <lacks>')."""
    if backend is None:
        backend = HipBackend(device)
    if flag is not None and not getattr(backend, flag, False):
        raise NotImplementedError(f'{getattr(backend, "name", type(backend).__name__)} {lacks}')
    return backend


class HipBackend:
    """Thin call surface over the C ABI; launches go to torch's current HIP stream of `device`."""
    name = 'hip'
    supports_tiled_grids = True      # d2d_cfg.grid_tile = 16 (the CPU oracle keeps the reference's row-major grids)
    supports_device_heading_gaze = True   # d2d_plan.gaze = LookAhead / LookGoal (the CPU oracle runs only Oxford's gaze stage)
    supports_device_owl_gaze = True       # d2d_plan.gaze = Owl
    supports_device_noise = True          # d2d_state.rng: the tracker stage draws the measurement noise itself (var_cam != 0)
    supports_device_worlds = True         # include/d2d_worlds.h: the seeded worlds are built on the device
    supports_vo_metric = True             # include/d2d_metrics.h: the velocity-obstacle feasibility metric (metrics.py)
    supports_difficulty_tables = True     # include/d2d_metrics.h: the traversability and survival-fit metrics (metrics.py)
    supports_rvo = True                   # include/d2d_rvo.h: the RVO motion profile (VecDrone2DEnv with motion_profile='RVO')
    supports_jerk = True                  # include/d2d_jerk.h: the Jerk_Primitive planner (VecDrone2DEnv with planner='Jerk_Primitive')
    supports_step_gaze = True             # include/d2d_gaze.h: LookAhead / Owl as a launch in front of the step (policy_step, run_episodes)
    supports_stepped_plugins = True       # include/d2d_stepped.h: the gaze and plan stages that leave finished envs alone (run_episodes)
    supports_rvo_live = True              # include/d2d_rvo_live.h: the RVO launches that leave finished envs alone (run_episodes)
    supports_seen_obs = True              # include/d2d_seen.h: the time-since-observed map and its crop (VecDrone2DEnv(..., seen_obs=True))
    supports_scan_obs = True              # include/d2d_scan.h: the per-ray scan of the raycast (VecDrone2DEnv(..., scan_obs=True))
    supports_tracks_obs = True            # include/d2d_tracks.h: the tracker-forecast map's window (VecDrone2DEnv(..., tracks_obs=True))
    supports_fork = True                  # include/d2d_fork.h: whole slot states copied in one launch (load_slots, fork, whatif.branch_terms)
    supports_render = True                # include/d2d_render.h: display lists and frames of any slots (render_list, render_frames)

    def __init__(self, device='cuda:0'):
        import torch
        if not torch.cuda.is_available():
            raise D2DError('HipBackend needs a GPU (torch.cuda.is_available() is False)')
        self.torch = torch
        self.device = torch.device(device)
        self.lib, self.fn = load_library()
        self.wpfn = A.bind_swept(self.lib)                                # include/d2d_swept.h, where the build has it
        self.wlib, self.wfn = load_worlds_library()
        self.sfn = A.bind_worlds_stream(self.wlib)                        # include/d2d_worlds_stream.h, where the build has it
        self.sfn.update(A.bind_worlds_table(self.wlib))                   # include/d2d_worlds_table.h, likewise
        self.sfn.update(A.bind_worlds_turn(self.wlib))                    # include/d2d_worlds_turn.h, likewise
        self.mlib = self.mfn = None       # libd2d_metrics.so: loaded by the first metric call, so that a tree without it runs the rest
        self.rlib = self.rfn = None       # libd2d_rvo.so: loaded by the first RVO call, likewise
        self.jlib = self.jfn = None       # libd2d_jerk.so: loaded by the first Jerk_Primitive call, likewise
        self.glib = self.gfn = None       # libd2d_gaze.so: loaded by the first gaze call of the step path, likewise
        self.olib = self.ofn = None       # libd2d_seen.so: loaded by the first update of the time-since-observed map, likewise
        self.ylib = self.yfn = None       # libd2d_scan.so: loaded by the first update of the per-ray scan, likewise
        self.tlib = self.tfn = None       # libd2d_tracks.so: loaded by the first update of the tracker-forecast map, likewise
        self.klib = self.kfn = None       # libd2d_fork.so: loaded by the first fork of slots, likewise
        self.vlib = self.vfn = None       # libd2d_render.so: loaded by the first render_list() / render_frames(), likewise

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, rc):
        _check(rc, self.fn, 'd2d')

    def run_stages(self, cfg, st, stages):
        self._chk(self.fn['run_stages'](C.byref(cfg), C.byref(st), stages, self._stream()))

    def step(self, cfg, st):
        self._chk(self.fn['step'](C.byref(cfg), C.byref(st), self._stream()))

    def perceive(self, cfg, st):
        self._chk(self.fn['perceive'](C.byref(cfg), C.byref(st), self._stream()))

    def act(self, cfg, st):
        self._chk(self.fn['act'](C.byref(cfg), C.byref(st), self._stream()))

    def rollout(self, cfg, st, nsteps, actions, pin=None, coll_out=None, wp_steps=None):
        self._chk(self.fn['rollout'](C.byref(cfg), C.byref(st), nsteps, actions.data_ptr(),
                                     None if wp_steps is None else wp_steps.data_ptr(),
                                     None if pin is None else pin.data_ptr(),
                                     None if coll_out is None else coll_out.data_ptr(), self._stream()))

    def reset(self, cfg, st, init, mask=None):
        self._chk(self.fn['reset'](C.byref(cfg), C.byref(st), C.byref(init),
                                   None if mask is None else mask.data_ptr(), self._stream()))

    def gaze_stage(self, cfg, st, plan):
        self._chk(self.fn['gaze_stage'](C.byref(cfg), C.byref(st), C.byref(plan), self._stream()))

    def plan_stage(self, cfg, st, plan):
        self._chk(self.fn['plan_stage'](C.byref(cfg), C.byref(st), C.byref(plan), self._stream()))

    def _stepped(self, name):
        if name not in self.fn:
            raise D2DError(f'{LIB_PATH} has no d2d_{name} (include/d2d_stepped.h): rebuild it with csrc/build.sh')
        return self.fn[name]

    def gaze_stage_live(self, cfg, st, plan):
        """d2d_gaze_stage_live: d2d_gaze_stage for the envs that are not done"""
        self._chk(self._stepped('gaze_stage_live')(C.byref(cfg), C.byref(st), C.byref(plan), self._stream()))

    def plan_stage_live(self, cfg, st, plan):
        """d2d_plan_stage_live: d2d_plan_stage for the envs that are not done"""
        self._chk(self._stepped('plan_stage_live')(C.byref(cfg), C.byref(st), C.byref(plan), self._stream()))

    @property
    def supports_swept_obs(self):
        """include/d2d_swept.h: the swept-trajectory map and its crop (VecDrone2DEnv(..., swept_obs=True)).  Optional symbols of
        libd2d_hip.so: true where the built library has both"""
        return all(n in self.wpfn for n in A.SWEPT_ENTRY_POINTS)

    def _swept(self, name):
        if name not in self.wpfn:
            raise D2DError(f'{LIB_PATH} has no d2d_{name} (include/d2d_swept.h): rebuild it with csrc/build.sh')
        return self.wpfn[name]

    def swept_mark(self, cfg, st, plan, sw):
        """d2d_swept_mark: the map replan_check is about to return, for the envs that are not done (between perceive and plan)"""
        self._chk(self._swept('swept_mark')(C.byref(cfg), C.byref(st), C.byref(plan), C.byref(sw), self._stream()))

    def swept_crop(self, cfg, st, sw):
        """d2d_swept_crop: the crop of that map around the drone's cell, for the envs the last mark ran for (after act)"""
        self._chk(self._swept('swept_crop')(C.byref(cfg), C.byref(st), C.byref(sw), self._stream()))

    def closed_loop(self, cfg, st, plan, nsteps, on_done=0, init=None):
        self._chk(self.fn['closed_loop'](C.byref(cfg), C.byref(st), C.byref(plan), nsteps, int(on_done),
                                         None if init is None else C.byref(init), self._stream()))

    def plan_reset(self, cfg, plan, mask=None, mask_stride=1):
        self._chk(self.fn['plan_reset'](C.byref(cfg), C.byref(plan), None if mask is None else mask.data_ptr(),
                                        mask_stride, self._stream()))

    def sincos_array(self, x, s, c):
        self._chk(self.fn['sincos_array'](x.data_ptr(), s.data_ptr(), c.data_ptr(), x.numel(), self._stream()))

    def atan2_array(self, y, x, out):
        self._chk(self.fn['atan2_array'](y.data_ptr(), x.data_ptr(), out.data_ptr(), y.numel(), self._stream()))

    def pow2_array(self, x, out):
        self._chk(self.fn['pow2_array'](x.data_ptr(), out.data_ptr(), x.numel(), self._stream()))

    def log_array(self, x, out):
        self._chk(self.fn['log_array'](x.data_ptr(), out.data_ptr(), x.numel(), self._stream()))

    def rng_draw(self, rng, m, out):
        """rng [B, RNG_WORDS] int32 / uint32 bits, m [B] int32, out [B, max_m, 2] float64"""
        self._chk(self.fn['rng_draw'](rng.data_ptr(), m.data_ptr(), out.data_ptr(), rng.shape[0], out.shape[1], self._stream()))

    def build_worlds(self, spec, st):
        """d2d_worlds_build: fill the world fields behind `st` for the envs of `spec` (vec_env.world_spec) on the current stream"""
        _check(self.wfn['build'](C.byref(spec), C.byref(st), self._stream()), self.wfn, 'd2d_worlds')

    @property
    def supports_episode_stream(self):
        """include/d2d_worlds_stream.h: the launches that refill finished slots with the next seeded episodes (stream_episodes).
        Optional symbols of libd2d_worlds.so: true where the built library has all of them"""
        return all(n in self.sfn for n in A.STREAM_ENTRY_POINTS)

    @property
    def supports_episode_table(self):
        """include/d2d_worlds_table.h: the assignment that hands a finished slot a row of an episode table
        (stream_episodes(episodes=...)).  An optional symbol of libd2d_worlds.so: true where the built library has it"""
        return all(n in self.sfn for n in A.TABLE_ENTRY_POINTS)

    def _stream_fn(self, name, *args):
        if name not in self.sfn:
            header = ('d2d_worlds_table.h' if name in A.TABLE_ENTRY_POINTS else
                      'd2d_worlds_turn.h' if name in A.TURN_ENTRY_POINTS else 'd2d_worlds_stream.h')
            raise D2DError(f'{WORLDS_LIB_PATH} has no d2d_{name} (include/{header}): rebuild it with csrc/worlds/build.sh')
        _check(self.sfn[name](*args, self._stream()), self.wfn, 'd2d_worlds')

    def stream_harvest(self, cfg, st, slot_episode, rows):
        """d2d_stream_harvest: every slot that is done and not retired writes its record to rows [M, 8] int32 at slot_episode[e]"""
        self._stream_fn('stream_harvest', C.byref(st), slot_episode.data_ptr(), slot_episode.shape[0], cfg.W, cfg.H, cfg.grid_tile,
                        rows.shape[0], rows.data_ptr())

    def stream_assign(self, flags, num_episodes, map_id0, slot_episode, map_id, refill, counts):
        """d2d_stream_assign: the slots just harvested get the next episodes in slot order (slot_episode, map_id, refill byte), or
        retire; counts [2] int64 = (cursor, finished) moves on"""
        self._stream_fn('stream_assign', flags.data_ptr(), slot_episode.shape[0], int(num_episodes), int(map_id0), slot_episode.data_ptr(),
                        map_id.data_ptr(), refill.data_ptr(), counts.data_ptr())

    def stream_assign_table(self, flags, ep_map_id, ep_par, ep_tgt, slot_episode, map_id, env_par, env_tgt, refill, counts):
        """d2d_stream_assign_table: stream_assign for a table of episodes -- a slot that gets episode k copies ep_map_id[k] ([M] uint32
        bits), ep_par[k] ([M, 8] float64) and ep_tgt[k] ([M, T, 2] float64) into its map_id, env_par and env_tgt"""
        self._stream_fn('stream_assign_table', flags.data_ptr(), slot_episode.shape[0], ep_map_id.shape[0], env_tgt.shape[1],
                        ep_map_id.data_ptr(), ep_par.data_ptr(), ep_tgt.data_ptr(), slot_episode.data_ptr(), map_id.data_ptr(),
                        env_par.data_ptr(), env_tgt.data_ptr(), refill.data_ptr(), counts.data_ptr())

    def build_worlds_masked(self, spec, st, refill):
        """d2d_worlds_build_masked: build_worlds for the slots with refill [B] uint8 set, nothing of any other slot"""
        self._stream_fn('worlds_build_masked', C.byref(spec), C.byref(st), refill.data_ptr())

    def stream_clear(self, t, refill):
        """d2d_stream_clear: rows e of the per-slot tensor t [B, ...] with refill [B] uint8 set become 0, nothing else is written"""
        if t.numel():
            self._stream_fn('stream_clear', t.data_ptr(), t[0].numel() * t.element_size(), refill.data_ptr(), t.shape[0])

    @property
    def supports_action_stream(self):
        """include/d2d_worlds_turn.h: the restore and the per-step count of a stream the caller steps itself (action_stream).
        Optional symbols of libd2d_worlds.so: true where the built library has both"""
        return all(n in self.sfn for n in A.TURN_ENTRY_POINTS)

    def stream_restore(self, items, n_items, refill):
        """d2d_stream_restore: `items` is a device tensor that holds n_items packed _abi.RestoreItem records
        (action_stream.pack_items); every item is applied to the slots with refill [B] uint8 set, nothing else is written"""
        self._stream_fn('stream_restore', items.data_ptr(), int(n_items), refill.data_ptr(), refill.shape[0])

    def stream_explored(self, cfg, st, cells):
        """d2d_stream_explored: cells [B] int32 = the non-zero cells of every slot's dmap, as stream_harvest counts them"""
        self._stream_fn('stream_explored', C.byref(st), cells.shape[0], cfg.W, cfg.H, cfg.grid_tile, cells.data_ptr())

    def _metrics(self, name, *args):
        if self.mfn is None:
            self.mlib, self.mfn = load_metrics_library()
        _check(self.mfn[name](*args, self._stream()), self.mfn, 'd2d_metrics')

    def vo_geometry(self, agents, pos, rA, arg, theta_ba, collided):
        """d2d_vo_geometry: agents [B, 6, N], pos [P, 2] -> arg, theta_ba [B, P, N] float64, collided [B, P] uint8"""
        B, _, N = agents.shape
        self._metrics('vo_geometry', agents.data_ptr(), pos.data_ptr(), float(rA), B, N, pos.shape[0], arg.data_ptr(),
                      theta_ba.data_ptr(), collided.data_ptr())

    def vo_cones(self, theta_ba, half, collided, cone):
        """d2d_vo_cones: theta_ba, half [B, P, N], collided [B, P] -> cone [B, P, N, 2] (theta_right, theta_left)"""
        B, P, N = theta_ba.shape
        self._metrics('vo_cones', theta_ba.data_ptr(), half.data_ptr(), collided.data_ptr(), B, N, P, cone.data_ptr())

    def vo_cones_arg(self, theta_ba, arg, collided, half, cone):
        """d2d_vo_cones_arg: theta_ba, arg [B, P, N], collided [B, P] -> half [B, P, N] (or None: not kept) and cone [B, P, N, 2];
        the half angle asin(arg) is taken on the device"""
        B, P, N = theta_ba.shape
        self._metrics('vo_cones_arg', theta_ba.data_ptr(), arg.data_ptr(), collided.data_ptr(), B, N, P,
                      None if half is None else half.data_ptr(), cone.data_ptr())

    def asin_array(self, x, out):
        """d2d_asin_array: out[i] = libm's asin(x[i]) on the device (NaN for |x| > 1); float64, out may be x"""
        self._metrics('asin_array', x.data_ptr(), x.numel(), out.data_ptr())

    def vo_count(self, agents, cand, cone, collided, count):
        """d2d_vo_count: agents [B, 6, N], cand [C, 2], cone, collided -> count [B, P] int32 (-1: collided position)"""
        B, P, N, _ = cone.shape
        self._metrics('vo_count', agents.data_ptr(), cand.data_ptr(), cone.data_ptr(), collided.data_ptr(), B, N, P, cand.shape[0],
                      count.data_ptr())

    def trav_steps(self, gt, starts, steps):
        """d2d_trav_steps: gt [B, W, H] uint8 (row-major), starts [S, 2] int32 (inside the grid: the caller has checked) ->
        steps [B, S, 8] int32 (-1: the start cell is not UNOCCUPIED)"""
        B, W, H = gt.shape
        self._metrics('trav_steps', gt.data_ptr(), B, W, H, starts.data_ptr(), starts.shape[0], steps.data_ptr())

    def fit_first_hit(self, agents, pos, drone_radius, W_px, H_px, scale, dt, checks, first, agents_out=None):
        """d2d_fit_first_hit: agents [B, 6, N], pos [P, 2] -> first [B, P] int32 (-1: never hit), agents_out [B, 6, N] or None"""
        B, _, N = agents.shape
        self._metrics('fit_first_hit', agents.data_ptr(), pos.data_ptr(), float(drone_radius), float(W_px), float(H_px), float(scale),
                      float(dt), B, N, pos.shape[0], int(checks), first.data_ptr(), None if agents_out is None else agents_out.data_ptr())

    def _rvo(self, name, *args):
        if self.rfn is None:
            self.rlib, self.rfn = load_rvo_library()
            self.rfn = dict(self.rfn, **A.bind_rvo_live(self.rlib))       # include/d2d_rvo_live.h, where the build has it
        if name not in self.rfn:
            raise D2DError(f'{RVO_LIB_PATH} has no d2d_rvo_{name} (include/d2d_rvo_live.h): rebuild it with csrc/rvo/build.sh')
        _check(self.rfn[name](*args, self._stream()), self.rfn, 'd2d_rvo')

    def rvo_velocity(self, agents, vel, pillars, vel_out):
        """d2d_rvo_velocity: agents [B, 6, N], vel [B, 2, N] float64, pillars [B, P, 3] int32 -> vel_out [B, 2, N] (not vel)"""
        B, _, N = agents.shape
        P = pillars.shape[1]
        self._rvo('velocity', agents.data_ptr(), vel.data_ptr(), pillars.data_ptr() if P else None, B, N, P, vel_out.data_ptr())

    def rvo_agents_step(self, agents, vel, W_px, H_px, scale, dt):
        """d2d_rvo_agents_step: Agent.step of agents [B, 6, N] in place, moving with vel [B, 2, N]"""
        B, _, N = agents.shape
        self._rvo('agents_step', agents.data_ptr(), vel.data_ptr(), float(W_px), float(H_px), float(scale), float(dt), B, N)

    def rvo_velocity_live(self, agents, vel, pillars, flags, vel_out):
        """d2d_rvo_velocity_live: rvo_velocity for the envs whose flags [B, 4] uint8 do not say done; a finished env's vel_out is its vel"""
        B, _, N = agents.shape
        P = pillars.shape[1]
        self._rvo('velocity_live', agents.data_ptr(), vel.data_ptr(), pillars.data_ptr() if P else None,
                  None if flags is None else flags.data_ptr(), B, N, P, vel_out.data_ptr())

    def rvo_agents_step_live(self, agents, vel, flags, W_px, H_px, scale, dt):
        """d2d_rvo_agents_step_live: rvo_agents_step for the envs whose flags do not say done; a finished env's agents stay"""
        B, _, N = agents.shape
        self._rvo('agents_step_live', agents.data_ptr(), vel.data_ptr(), None if flags is None else flags.data_ptr(), float(W_px),
                  float(H_px), float(scale), float(dt), B, N)

    def _jerk_fn(self):
        if self.jfn is None:
            self.jlib, self.jfn = load_jerk_library()
            self.jfn = dict(self.jfn, **A.bind_jerk_live(self.jlib))      # include/d2d_jerk_live.h, where the build has it
        return self.jfn

    def _jerk(self, name, *args):
        fn = self._jerk_fn()
        if name not in fn:
            raise D2DError(f'{JERK_LIB_PATH} has no d2d_jerk_{name} (include/d2d_jerk_live.h): rebuild it with csrc/jerk/build.sh')
        _check(fn[name](*args, self._stream()), fn, 'd2d_jerk')

    @property
    def supports_jerk_live(self):
        """include/d2d_jerk_live.h: the plan launch that leaves finished envs alone (run_episodes).  An optional symbol of
        libd2d_jerk.so: true where the built library has it"""
        return 'plan_live' in self._jerk_fn()

    def jerk_plan(self, call):
        """d2d_jerk_plan: `call` is an _abi.JerkCall of device pointers (jerk_plugin.JerkState.call)"""
        self._jerk('plan', C.byref(call))

    def jerk_plan_live(self, call, flags):
        """d2d_jerk_plan_live: jerk_plan for the envs whose flags [B, 4] uint8 do not say done; nothing of a finished env is written"""
        self._jerk('plan_live', C.byref(call), None if flags is None else flags.data_ptr())

    def jerk_reset(self, trk_radius, trk_prev, trk_radius0, mask=None, mask_stride=1):
        """d2d_jerk_reset: trk_radius [B, N] float64 <- trk_radius0, trk_prev [B, N] uint8 <- 0, for the envs of mask (or all)"""
        B, N = trk_radius.shape
        self._jerk('reset', trk_radius.data_ptr(), trk_prev.data_ptr(), trk_radius0.data_ptr(),
                   None if mask is None else mask.data_ptr(), int(mask_stride), B, N)

    def _gaze(self, name, *args):
        if self.gfn is None:
            self.glib, self.gfn = load_gaze_library()
        _check(self.gfn[name](*args, self._stream()), self.gfn, 'd2d_gaze')

    def gaze_act(self, call):
        """d2d_gaze_act: `call` is an _abi.GazeCall of device pointers (gaze_plugin.GazeState.call)"""
        self._gaze('act', C.byref(call))

    def gaze_reset(self, owl_state, mask=None, mask_stride=1):
        """d2d_gaze_reset: owl_state [B, OWL_STATE_F] float64 <- 0, for the envs of mask (or all)"""
        self._gaze('reset', owl_state.data_ptr(), None if mask is None else mask.data_ptr(), int(mask_stride), owl_state.shape[0])

    def seen_update(self, cfg, st, seen):
        """d2d_seen_update: `seen` is an _abi.Seen of device pointers (VecDrone2DEnv(..., seen_obs=True)); the envs whose step counter
        has moved since their latest update get their map marked from the pose they are in, and its crop"""
        if self.ofn is None:
            self.olib, self.ofn = load_seen_library()
        _check(self.ofn['update'](C.byref(cfg), C.byref(st), C.byref(seen), self._stream()), self.ofn, 'd2d_seen')

    def scan_update(self, cfg, st, scan):
        """d2d_scan_update: `scan` is an _abi.Scan of device pointers (VecDrone2DEnv(..., scan_obs=True)); the envs whose step counter
        has moved since their latest update get the rays of that step, cast from the pose snapshot over the agents as they stand"""
        if self.yfn is None:
            self.ylib, self.yfn = load_scan_library()
        _check(self.yfn['update'](C.byref(cfg), C.byref(st), C.byref(scan), self._stream()), self.yfn, 'd2d_scan')

    def tracks_update(self, cfg, st, tracks):
        """d2d_tracks_update: `tracks` is an _abi.Tracks of device pointers (VecDrone2DEnv(..., tracks_obs=True)); the envs whose step
        counter differs from that of their latest update (all of them with `force`) get the window of the tracker-forecast map"""
        if self.tfn is None:
            self.tlib, self.tfn = load_tracks_library()
        _check(self.tfn['update'](C.byref(cfg), C.byref(st), C.byref(tracks), self._stream()), self.tfn, 'd2d_tracks')

    def fork_slots(self, items, n_items, src_of, B_src, in_place, status):
        """d2d_fork_slots: `items` is a device tensor that holds n_items packed _abi.ForkItem records (fork.pack_items); slot e of the
        destination buffers becomes slot src_of[e] ([B_dst] int32) of the source buffers ([B_src] slots), status [B_dst] uint8 says
        what happened to it (FORK_LEFT / FORK_COPIED / FORK_REFUSED).  No host read"""
        if self.kfn is None:
            self.klib, self.kfn = load_fork_library()
        _check(self.kfn['slots'](items.data_ptr() if n_items else None, int(n_items), src_of.data_ptr(), src_of.shape[0], int(B_src),
                                 int(bool(in_place)), status.data_ptr(), self._stream()), self.kfn, 'd2d_fork')

    def _render_fn(self):
        if self.vfn is None:
            self.vlib, self.vfn = load_render_library()
            self.vfn = dict(self.vfn, **A.bind_capture(self.vlib))        # include/d2d_capture.h, where the build has it
        return self.vfn

    def _render(self, name, *args):
        fn = self._render_fn()
        if name not in fn:
            raise D2DError(f'{RENDER_LIB_PATH} has no d2d_{name} (include/d2d_capture.h): rebuild it with csrc/render/build.sh')
        _check(fn[name](*args, self._stream()), fn, 'd2d_render')

    @property
    def supports_capture(self):
        """include/d2d_capture.h: the selection and the two skipping launches behind capture.Capture.  Optional symbols of
        libd2d_render.so: true where the built library has all three"""
        return all(n in self._render_fn() for n in A.CAPTURE_ENTRY_POINTS)

    def capture_select(self, cfg, st, slot_episode, kinds, sel_slot, sel_dst, meta, pose, counts):
        """d2d_capture_select: the finished slots of the kinds in the bit mask `kinds` that the next harvest records (slot_episode
        None: every done slot, episode = slot) get the next rows of meta [capacity, 4] int32 and pose [capacity, 3] float64; sel_slot
        and sel_dst [S] int32 name them for the two launches below, -1 beyond; counts [3] int64 = (taken, dropped, matched) moves on"""
        self._render('capture_select', C.byref(cfg), C.byref(st), None if slot_episode is None else slot_episode.data_ptr(), int(kinds),
                     sel_slot.shape[0], meta.shape[0], sel_slot.data_ptr(), sel_dst.data_ptr(), meta.data_ptr(), pose.data_ptr(),
                     counts.data_ptr())

    def render_list_sel(self, cfg, st, call):
        """d2d_render_list_sel: render_list, an entry whose slot is -1 skipped (status RENDER_SKIPPED)"""
        self._render('render_list_sel', C.byref(cfg), C.byref(st), C.byref(call))

    def render_frame_sel(self, cfg, st, call, dst, capacity):
        """d2d_render_frame_sel: render_frame with entry i painted into frame dst[i] ([S] int32) of call.frame [capacity, Hf, Wf, 3];
        skipped entries and those with dst outside [0, capacity) paint nothing"""
        self._render('render_frame_sel', C.byref(cfg), C.byref(st), C.byref(call), dst.data_ptr(), int(capacity))

    def render_list(self, cfg, st, call):
        """d2d_render_list: `call` is an _abi.RenderCall of device pointers (VecDrone2DEnv.render_list); the display lists of its slots"""
        self._render('list', C.byref(cfg), C.byref(st), C.byref(call))

    def render_frame(self, cfg, st, call):
        """d2d_render_frame: the frames of the call's slots from the lists render_list left in its buffers and from the drone's map"""
        self._render('frame', C.byref(cfg), C.byref(st), C.byref(call))

    def render_raster(self, call):
        """d2d_render_raster (include/d2d_render_hooks.h): `call` is an _abi.RasterCall over a caller-made list and cell layer"""
        self._render('raster', C.byref(call))

    def tan_array(self, x, out):
        self._chk(self.fn['tan_array'](x.data_ptr(), out.data_ptr(), x.numel(), self._stream()))

    def sync(self):
        self.torch.cuda.synchronize(self.device)
