"""ctypes mirror of include/d2d.h (the C ABI of the HIP library).  Field order and types must match
the header exactly; tests/test_abi.py cross-checks sizes and constants against the header text."""
import ctypes as C

D2D_ABI_VERSION = 8

UNEXPLORED, OCCUPIED, UNOCCUPIED, DYNAMIC = 0, 1, 2, 3
SM_WAIT_FOR_GOAL, SM_GOAL_REACHED, SM_PLANNING, SM_EXECUTING = 0, 1, 2, 3
PLANNER_EXTERNAL, PLANNER_NOMOVE = 0, 1
PLAN_NONE, PLAN_PRIMITIVE = 0, 1
GAZE_NONE, GAZE_OXFORD = 0, 1
GAZE_LOOKAHEAD, GAZE_LOOKGOAL = 2, 3   # yaw_planner.py:18-39 / :225-257 on the device
GAZE_OWL = 5                           # yaw_planner.py:151-222 on the device (4 is unassigned)
# d2d_plan.owl_tab / owl_state layouts (include/d2d.h D2D_OWL_*)
OWL_NRATE, OWL_NDIR = 20, 36
OWL_T_RATE, OWL_T_RATE08, OWL_T_TURN, OWL_T_ACT, OWL_T_DIR, OWL_T_FOV, OWL_T_DEPTH, OWL_T_HOLD, OWL_TAB_LEN = 0, 20, 40, 60, 80, 152, 153, 154, 160
OWL_STATE_F, OWL_S_RATE, OWL_S_LEFT = 40, 36, 37
NODE_F = 12

AF = 6
A_PX, A_PY, A_VX, A_VY, A_R, A_R2 = range(6)
DF = 8
D_X, D_Y, D_YAW, D_VX, D_VY, D_AX, D_AY, D_PAD = range(8)
CF = 8
C_STEPS, C_FAIL, C_SM, C_TGT_NEXT, C_NTGT, C_TRACKED, C_BUF_N, C_BUF_TS = range(8)
F_COLLISION, F_DEADLOCK, F_FREEZING, F_DONE = range(4)
KF = 20
RNG_WORDS, RNG_POS, RNG_NPAIR, RNG_NREGEN = 640, 624, 625, 626   # d2d_state.rng (include/d2d.h D2D_RNG_WORDS)

ST_FSM, ST_AGENTS, ST_RAYCAST, ST_DYNGRID, ST_TRACKER, ST_CONTROL, ST_COLLIDE, ST_OBS = (1 << i for i in range(8))
ST_PERCEIVE = ST_FSM | ST_AGENTS | ST_RAYCAST | ST_DYNGRID | ST_TRACKER
ST_ACT = ST_CONTROL | ST_COLLIDE | ST_OBS
ST_ALL = ST_PERCEIVE | ST_ACT
ST_SKIP_DONE = 256
DONE_CONTINUE, DONE_RESET, DONE_FREEZE = 0, 1, 2


class Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ('abi_version', 'B', 'N', 'W', 'H', 'R', 'L', 'T', 'planner_mode', 'kf_enabled',
                 'noise_rows', 'noise_row0', 'grid_tile', 'reserved2')] + \
               [(n, C.c_double) for n in
                ('dt', 'scale', 'W_px', 'H_px', 'ray_off0', 'ray_dth', 'depth', 'drone_radius', 'yaw_rate',
                 'max_acc', 'max_steps', 'sigma', 'kf_lo_x', 'kf_hi_x', 'kf_lo_y', 'kf_hi_y')]


STATE_FIELDS = ('agents', 'agent_unit', 'dyn_prev', 'gt', 'dmap', 'drone', 'target', 'targets', 'counters',
                'active', 'kf', 'kf_len', 'action', 'plan_ok', 'wp_valid', 'wp', 'noise', 'hit', 'newly',
                'flags', 'obs_local', 'obs_yaw', 'rng', 'rng_draws')


class State(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STATE_FIELDS]


PLAN_INT_FIELDS = ('planner', 'gaze', 'nu', 'n_sample', 'n_ts', 'max_itr', 'traj_cap', 'node_cap', 'hash_cap', 'n_yaw',
                   'pw_nleaf', 'pw_nprog', 'tobs_len', 'pw_ntree')
PLAN_F64_FIELDS = ('horizon', 'vmax', 'safe_dist', 'goal_tol', 'agent_radius', 'half_fov', 'yaw_rate_max', 'vmax_sq', 'goal_sq')
PLAN_TABLES = ('u_space', 'sample_t', 'traj_t', 'yaw_space', 'tobs_tab', 'pw_leaf', 'pw_prog', 'pw_tree', 'pw_rowleaf', 'trk_radius0', 'owl_tab')
PLAN_STATE = ('traj', 'traj_hdr', 'traj_box', 'trk_radius', 'trk_prev', 'trk_lim', 'seen_step', 'nodes', 'hash', 'launch_args', 'plan_stat', 'owl_state')
LAUNCH_ARGS_BYTES = 2048


class Plan(C.Structure):
    """include/d2d.h `d2d_plan`."""
    _fields_ = [(n, C.c_int32) for n in PLAN_INT_FIELDS] + [(n, C.c_double) for n in PLAN_F64_FIELDS] + \
               [('acos_key_lo', C.c_int64), ('acos_mask', C.c_uint64)] + \
               [(n, C.c_void_p) for n in PLAN_TABLES + PLAN_STATE]


def bind(lib, prefix='d2d_'):
    """Declare argtypes / restypes of every entry point of include/d2d.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'abi_version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'step': (C.c_int, [P(Cfg), P(State), C.c_void_p]),
        'perceive': (C.c_int, [P(Cfg), P(State), C.c_void_p]),
        'act': (C.c_int, [P(Cfg), P(State), C.c_void_p]),
        'run_stages': (C.c_int, [P(Cfg), P(State), C.c_uint32, C.c_void_p]),
        'rollout': (C.c_int, [P(Cfg), P(State), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        'reset': (C.c_int, [P(Cfg), P(State), P(State), C.c_void_p, C.c_void_p]),
        'tan_array': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        'gaze_stage': (C.c_int, [P(Cfg), P(State), P(Plan), C.c_void_p]),
        'plan_stage': (C.c_int, [P(Cfg), P(State), P(Plan), C.c_void_p]),
        'closed_loop': (C.c_int, [P(Cfg), P(State), P(Plan), C.c_int32, C.c_int32, P(State), C.c_void_p]),
        'plan_reset': (C.c_int, [P(Cfg), P(Plan), C.c_void_p, C.c_int32, C.c_void_p]),
        'sincos_array': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        'atan2_array': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        'pow2_array': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        'log_array': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
        'rng_draw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
        'launch_shape': (C.c_int, [P(Cfg), P(Plan), P(C.c_int32 * 4)]),
        'gaze_stage_live': (C.c_int, [P(Cfg), P(State), P(Plan), C.c_void_p]),
        'plan_stage_live': (C.c_int, [P(Cfg), P(State), P(Plan), C.c_void_p]),
    }
    return _bind(lib, prefix, sig, OPTIONAL)


def _bind(lib, prefix, sig, optional=()):
    """key -> the entry point `prefix + key` of `lib` with the (restype, argtypes) of `sig` declared on it"""
    out = {}
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(lib, prefix + name):
            continue                       # a diagnostic query older builds of the library lack (A/B runs via D2D_LIB)
        fn = getattr(lib, prefix + name)   # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
        out[name] = fn
    return out


# atan2_array, pow2_array, log_array, rng_draw: test hooks of the HIP library alone (include/d2d_hooks.h), outside the surface the
# oracle mirrors
# gaze_stage_live, plan_stage_live: include/d2d_stepped.h, the stages of the HIP library for the step path's episode loop (additions:
# an older build of the library, or the oracle, has none, and HipBackend.supports_stepped_plugins asks for them by name)
OPTIONAL = ('launch_shape', 'atan2_array', 'pow2_array', 'log_array', 'rng_draw', 'gaze_stage_live', 'plan_stage_live')
HIP_ONLY_ENTRY_POINTS = ('atan2_array', 'pow2_array', 'log_array', 'rng_draw')
STEPPED_ENTRY_POINTS = ('gaze_stage_live', 'plan_stage_live')
ENTRY_POINTS = ('abi_version', 'last_error', 'step', 'perceive', 'act', 'run_stages', 'rollout', 'reset',
                'tan_array', 'gaze_stage', 'plan_stage', 'closed_loop', 'plan_reset', 'sincos_array', 'launch_shape')


# ---- include/d2d_swept.h: the swept-trajectory map of the Primitive planner as an observation (additions to libd2d_hip.so) ----
SWEPT_ENTRY_POINTS = ('swept_mark', 'swept_crop')
SWEPT_FIELDS = ('map', 'obs', 'count', 'live')
SWEPT_MAX_SIDE = 256


class Swept(C.Structure):
    """include/d2d_swept.h `d2d_swept`."""
    _fields_ = [(n, C.c_void_p) for n in SWEPT_FIELDS]


def bind_swept(lib, prefix='d2d_'):
    """argtypes / restypes of include/d2d_swept.h on the loaded libd2d_hip.so: additions to that library, looked up as optional
    symbols (a build without them binds nothing here, and its ABI version is the same)."""
    P, V = C.POINTER, C.c_void_p
    sig = {
        'swept_mark': (C.c_int, [P(Cfg), P(State), P(Plan), P(Swept), V]),
        'swept_crop': (C.c_int, [P(Cfg), P(State), P(Swept), V]),
    }
    return _bind(lib, prefix, sig, SWEPT_ENTRY_POINTS)


# ---- include/d2d_worlds.h: the world construction on the device (csrc/worlds/libd2d_worlds.so, its own version) ----
D2D_WORLDS_VERSION = 1
WORLDS_ENV_F = 8
WE_R_LO, WE_R_W, WE_SPEED, WE_TRK_R, WE_X0, WE_Y0, WE_NTGT, WE_REDRAW = range(8)
WORLDS_MAX_ATTEMPTS = 65536
WORLD_OK, WORLD_CAP = 0, 1
WORLD_SPEC_INT_FIELDS = ('version', 'B', 'N', 'n_rand', 'n_cells', 'P', 'T', 'W_px', 'H_px', 'scale', 'W', 'H', 'grid_tile',
                         'max_attempts')
WORLD_SPEC_F64_FIELDS = ('start_clear', 'pillar_clear')
WORLD_SPEC_POINTERS = ('unit', 'cells', 'map_id', 'env_par', 'env_tgt', 'tracker_radius', 'obstacles', 'status')


class WorldSpec(C.Structure):
    """include/d2d_worlds.h `d2d_world_spec`."""
    _fields_ = [(n, C.c_int32) for n in WORLD_SPEC_INT_FIELDS] + [(n, C.c_double) for n in WORLD_SPEC_F64_FIELDS] + \
               [(n, C.c_void_p) for n in WORLD_SPEC_POINTERS]


def bind_worlds(lib):
    """argtypes / restypes of include/d2d_worlds.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'build': (C.c_int, [P(WorldSpec), P(State), C.c_void_p]),
        'launch_shape': (C.c_int, [P(WorldSpec), P(C.c_int32 * 2)]),
    }
    return _bind(lib, 'd2d_worlds_', sig)


# include/d2d_worlds_stream.h: the launches that refill the finished slots of a resident batch with the next seeded episodes
STREAM_F_DONE = F_DONE         # D2D_STREAM_F_DONE
STREAM_ROW_F = 8
STREAM_R_STEPS, STREAM_R_SM, STREAM_R_BUF_N, STREAM_R_BUF_TS, STREAM_R_FLAG0, STREAM_R_DMAP = 0, 1, 2, 3, 4, 7
STREAM_BUILD_FAILED = 0        # column STREAM_R_STEPS of an episode whose world hit max_attempts
STREAM_MAX_EPISODES = 0x0fffffff
STREAM_ENTRY_POINTS = ('stream_harvest', 'stream_assign', 'worlds_build_masked', 'stream_clear')


def bind_worlds_stream(lib):
    """argtypes / restypes of include/d2d_worlds_stream.h on the loaded libd2d_worlds.so: additions to that library, looked up as
    optional symbols (a build without them binds nothing here, and its version is the same)."""
    P, V, I = C.POINTER, C.c_void_p, C.c_int32
    sig = {
        'stream_harvest': (C.c_int, [P(State), V, I, I, I, I, C.c_int64, V, V]),
        'stream_assign': (C.c_int, [V, I, C.c_int64, C.c_uint32, V, V, V, V, V]),
        'worlds_build_masked': (C.c_int, [P(WorldSpec), P(State), V, V]),
        'stream_clear': (C.c_int, [V, C.c_int64, V, I, V]),
    }
    return _bind(lib, 'd2d_', sig, STREAM_ENTRY_POINTS)


# include/d2d_worlds_table.h: the assignment of a stream whose episodes are the rows of a table
TABLE_ENTRY_POINTS = ('stream_assign_table',)


def bind_worlds_table(lib):
    """argtypes / restypes of include/d2d_worlds_table.h on the loaded libd2d_worlds.so: an addition to that library, looked up as
    an optional symbol (a build without it binds nothing here, and its version is the same)."""
    V, I = C.c_void_p, C.c_int32
    sig = {'stream_assign_table': (C.c_int, [V, I, C.c_int64, I, V, V, V, V, V, V, V, V, V, V])}
    return _bind(lib, 'd2d_', sig, TABLE_ENTRY_POINTS)


# include/d2d_worlds_turn.h: the turn of a stream the caller steps itself (VecDrone2DEnv.action_stream)
RESTORE_MAX_ITEMS, RESTORE_PARTS = 32, 8
RESTORE_ZERO, RESTORE_COPY = 0, 1
TURN_ENTRY_POINTS = ('stream_restore', 'stream_explored')


class RestoreItem(C.Structure):
    """include/d2d_worlds_turn.h `d2d_restore_item`."""
    _fields_ = [('dst', C.c_void_p), ('src', C.c_void_p)] + \
               [(n, C.c_int64) for n in ('dst_stride', 'src_stride', 'dst_off', 'src_off', 'bytes')] + \
               [('kind', C.c_int32), ('reserved', C.c_int32)]


def bind_worlds_turn(lib):
    """argtypes / restypes of include/d2d_worlds_turn.h on the loaded libd2d_worlds.so: additions to that library, looked up as
    optional symbols (a build without them binds nothing here, and its version is the same)."""
    P, V, I = C.POINTER, C.c_void_p, C.c_int32
    sig = {
        'stream_restore': (C.c_int, [V, I, V, I, V]),
        'stream_explored': (C.c_int, [P(State), I, I, I, I, V, V]),
    }
    return _bind(lib, 'd2d_', sig, TURN_ENTRY_POINTS)


# ---- include/d2d_metrics.h: the difficulty metrics on the device (csrc/metrics/libd2d_metrics.so, its own version) ----
D2D_METRICS_VERSION = 2
VO_MAX_B, VO_MAX_P, VO_MAX_ELEMS = 65535, 64 * 65535, 0x7fffffff
TRAV_MAX_ELEMS = 0x7fffffff
FIT_MAX_N, FIT_MAX_P, FIT_MAX_ELEMS = 256, 64 * 65535, 0x7fffffff


def bind_metrics(lib):
    """argtypes / restypes of include/d2d_metrics.h on a loaded CDLL."""
    V, I = C.c_void_p, C.c_int32
    own = {'version': (C.c_int, []), 'last_error': (C.c_char_p, [])}
    sig = {
        'vo_geometry': (C.c_int, [V, V, C.c_double, I, I, I, V, V, V, V]),
        'vo_cones': (C.c_int, [V, V, V, I, I, I, V, V]),
        'vo_cones_arg': (C.c_int, [V, V, V, I, I, I, V, V, V]),
        'vo_count': (C.c_int, [V, V, V, V, I, I, I, I, V, V]),
        'asin_array': (C.c_int, [V, C.c_int64, V, V]),
        'trav_steps': (C.c_int, [V, I, I, I, V, I, V, V]),
        'fit_first_hit': (C.c_int, [V, V, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, I, I, I, I, V, V, V]),
    }
    return dict(_bind(lib, 'd2d_metrics_', own), **_bind(lib, 'd2d_', sig))


# ---- include/d2d_rvo.h: the RVO motion profile on the device (csrc/rvo/libd2d_rvo.so, its own version) ----
D2D_RVO_VERSION = 1
RVO_MAX_CONES, RVO_MAX_ELEMS = 1024, 0x7fffffff


def bind_rvo(lib):
    """argtypes / restypes of include/d2d_rvo.h on a loaded CDLL."""
    V, I, D = C.c_void_p, C.c_int32, C.c_double
    own = {'version': (C.c_int, []), 'last_error': (C.c_char_p, [])}
    sig = {
        'velocity': (C.c_int, [V, V, V, I, I, I, V, V]),
        'agents_step': (C.c_int, [V, V, D, D, D, D, I, I, V]),
    }
    return _bind(lib, 'd2d_rvo_', dict(own, **sig))


RVO_LIVE_F_DONE = F_DONE       # include/d2d_rvo_live.h D2D_RVO_LIVE_F_DONE
RVO_LIVE_ENTRY_POINTS = ('velocity_live', 'agents_step_live')


def bind_rvo_live(lib):
    """argtypes / restypes of include/d2d_rvo_live.h on the loaded libd2d_rvo.so: additions to that library, looked up as optional
    symbols (a build without them binds nothing here, and its version is the same)."""
    V, I, D = C.c_void_p, C.c_int32, C.c_double
    sig = {
        'velocity_live': (C.c_int, [V, V, V, V, I, I, I, V, V]),
        'agents_step_live': (C.c_int, [V, V, V, D, D, D, D, I, I, V]),
    }
    return _bind(lib, 'd2d_rvo_', sig, RVO_LIVE_ENTRY_POINTS)


# ---- include/d2d_jerk.h: the Jerk_Primitive planner on the device (csrc/jerk/libd2d_jerk.so, its own version) ----
D2D_JERK_VERSION = 1
JERK_NTHETA, JERK_PATTERNS, JERK_MAX_S, JERK_MAX_N, JERK_TH_F, JERK_TT_F = 72, 288, 128, 1024, 8, 5
JERK_STAT_TIE, JERK_STAT_UNKNOWN, JERK_STAT_SHIFT = 1, 2, 8
JERK_CALL_POINTERS = ('drone', 'target', 'active', 'kf', 'dmap', 'trk_radius', 'trk_prev', 'th_tab', 'tt_tab', 'tie_perm', 'tie_eq',
                      'plan_ok', 'wp_valid', 'wp', 'choice', 'stat')
JERK_CALL_INT_FIELDS = ('B', 'N', 'S', 'W', 'H', 'grid_tile')
JERK_CALL_F64_FIELDS = ('scale', 'W_px', 'H_px', 'drone_radius', 'agent_radius', 'var_cam', 'half_v_max')


class JerkCall(C.Structure):
    """include/d2d_jerk.h `d2d_jerk_call`."""
    _fields_ = [(n, C.c_void_p) for n in JERK_CALL_POINTERS] + [(n, C.c_int32) for n in JERK_CALL_INT_FIELDS] + \
               [(n, C.c_double) for n in JERK_CALL_F64_FIELDS]


def bind_jerk(lib):
    """argtypes / restypes of include/d2d_jerk.h on a loaded CDLL."""
    V, I = C.c_void_p, C.c_int32
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'plan': (C.c_int, [C.POINTER(JerkCall), V]),
        'reset': (C.c_int, [V, V, V, V, I, I, I, V]),
    }
    return _bind(lib, 'd2d_jerk_', sig)


JERK_LIVE_F_DONE = F_DONE      # include/d2d_jerk_live.h D2D_JERK_LIVE_F_DONE
JERK_LIVE_ENTRY_POINTS = ('plan_live',)


def bind_jerk_live(lib):
    """argtypes / restypes of include/d2d_jerk_live.h on the loaded libd2d_jerk.so: an addition to that library, looked up as an
    optional symbol (a build without it binds nothing here, and its version is the same)."""
    sig = {'plan_live': (C.c_int, [C.POINTER(JerkCall), C.c_void_p, C.c_void_p])}
    return _bind(lib, 'd2d_jerk_', sig, JERK_LIVE_ENTRY_POINTS)


# ---- include/d2d_gaze.h: the gaze decision of the step path on the device (csrc/gaze/libd2d_gaze.so, its own version) ----
D2D_GAZE_VERSION = 1
GAZE_K_LOOKAHEAD, GAZE_K_OWL = GAZE_LOOKAHEAD, GAZE_OWL
GAZE_MAX_N = 1024
GAZE_CALL_POINTERS = ('drone', 'target', 'active', 'kf', 'flags', 'owl_state', 'owl_tab', 'action')
GAZE_CALL_INT_FIELDS = ('B', 'N', 'kind', 'reserved')
GAZE_CALL_F64_FIELDS = ('dt', 'yaw_rate_max')


class GazeCall(C.Structure):
    """include/d2d_gaze.h `d2d_gaze_call`."""
    _fields_ = [(n, C.c_void_p) for n in GAZE_CALL_POINTERS] + [(n, C.c_int32) for n in GAZE_CALL_INT_FIELDS] + \
               [(n, C.c_double) for n in GAZE_CALL_F64_FIELDS]


def bind_gaze(lib):
    """argtypes / restypes of include/d2d_gaze.h on a loaded CDLL."""
    V, I = C.c_void_p, C.c_int32
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'act': (C.c_int, [C.POINTER(GazeCall), V]),
        'reset': (C.c_int, [V, V, I, I, V]),
    }
    return _bind(lib, 'd2d_gaze_', sig)


# ---- include/d2d_seen.h: the time-since-observed map as an observation (csrc/seen/libd2d_seen.so, its own version) ----
D2D_SEEN_VERSION = 1
SEEN_POINTERS = ('seen', 'last_call', 'refreshed', 'obs', 'tab')
SEEN_BUFFERS = ('seen', 'last_call', 'refreshed', 'obs')      # per env; `tab` is the host's table


class Seen(C.Structure):
    """include/d2d_seen.h `d2d_seen`."""
    _fields_ = [(n, C.c_void_p) for n in SEEN_POINTERS] + [('acos_key_lo', C.c_int64), ('acos_mask', C.c_uint64)] + \
               [('tab_len', C.c_int32), ('reserved', C.c_int32)]


def bind_seen(lib):
    """argtypes / restypes of include/d2d_seen.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'update': (C.c_int, [P(Cfg), P(State), P(Seen), C.c_void_p]),
    }
    return _bind(lib, 'd2d_seen_', sig)


# ---- include/d2d_scan.h: the per-ray scan of the raycast (csrc/scan/libd2d_scan.so, its own version) ----
D2D_SCAN_VERSION = 1
SCAN_POINTERS = ('pose', 'end', 'kind', 'hit', 'obs', 'last_step')
SCAN_OUTPUTS = ('end', 'kind', 'hit', 'obs', 'last_step')     # what a reset or a refill clears; `pose` is the caller's snapshot


class Scan(C.Structure):
    """include/d2d_scan.h `d2d_scan`."""
    _fields_ = [(n, C.c_void_p) for n in SCAN_POINTERS] + [('hit_words', C.c_int32), ('reserved', C.c_int32)]


def bind_scan(lib):
    """argtypes / restypes of include/d2d_scan.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'update': (C.c_int, [P(Cfg), P(State), P(Scan), C.c_void_p]),
    }
    return _bind(lib, 'd2d_scan_', sig)


# ---- include/d2d_tracks.h: the tracker-forecast map as an observation (csrc/tracks/libd2d_tracks.so, its own version) ----
D2D_TRACKS_VERSION = 1
TRACKS_MAX_SAMPLES = 255
TRACKS_POINTERS = ('trk_radius', 'win', 'cells', 'last_step')
TRACKS_BUFFERS = ('win', 'cells', 'last_step')               # per env, the channel's own; `trk_radius` is the device planner's


class Tracks(C.Structure):
    """include/d2d_tracks.h `d2d_tracks`."""
    _fields_ = [(n, C.c_void_p) for n in TRACKS_POINTERS] + [('margin', C.c_double), ('samples', C.c_int32), ('force', C.c_int32)]


def bind_tracks(lib):
    """argtypes / restypes of include/d2d_tracks.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'update': (C.c_int, [P(Cfg), P(State), P(Tracks), C.c_void_p]),
    }
    return _bind(lib, 'd2d_tracks_', sig)


# ---- include/d2d_fork.h: whole slot states copied between envs or inside one (csrc/fork/libd2d_fork.so, its own version) ----
D2D_FORK_VERSION = 1
FORK_MAX_ITEMS, FORK_PARTS, FORK_SMALL_BYTES = 64, 8, 4096
FORK_LEFT, FORK_COPIED, FORK_REFUSED = 0, 1, 2


class ForkItem(C.Structure):
    """include/d2d_fork.h `d2d_fork_item`."""
    _fields_ = [('dst', C.c_void_p), ('src', C.c_void_p)] + [(n, C.c_int64) for n in ('dst_stride', 'src_stride', 'bytes')]


def bind_fork(lib):
    """argtypes / restypes of include/d2d_fork.h on a loaded CDLL."""
    V, I = C.c_void_p, C.c_int32
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'slots': (C.c_int, [V, I, V, I, I, I, V, V]),
    }
    return _bind(lib, 'd2d_fork_', sig)


# ---- include/d2d_render.h, include/d2d_render_hooks.h: the renderer (csrc/render/libd2d_render.so, its own version) ----
D2D_RENDER_VERSION = 1
RK_DISC, RK_LINE, RK_ARC, RK_POLY = 1, 2, 3, 4
RENDER_GEOM, RENDER_FIXED, RENDER_MAX_DOWNSAMPLE = 20, 10, 64
RENDER_OK, RENDER_OVERFLOW, RENDER_BAD_SLOT = 0, 1, 2
RENDER_ITEM_BYTES = 176
RENDER_CALL_POINTERS = ('slots', 'pillars', 'agent_vel', 'plan_traj', 'plan_hdr', 'traj', 'traj_len', 'items', 'bbox', 'count', 'status',
                        'frame')
RENDER_CALL_INTS = ('S', 'P', 'K', 'plan_cap', 'cap', 'n_seeded', 'downsample', 'reserved')
RASTER_CALL_POINTERS = ('items', 'count', 'cells', 'bbox', 'frame')
RASTER_CALL_INTS = ('S', 'cap', 'W', 'H', 'W_px', 'H_px', 'scale', 'downsample')


def render_cap(P, N, K):
    """D2D_RENDER_CAP: the items of a slot with P pillars, N agents and a trajectory of at most K positions"""
    return RENDER_FIXED + int(P) + 2 * int(N) + (int(K) - 1 if K > 1 else 0)


class RenderItem(C.Structure):
    """include/d2d_render.h `d2d_render_item`."""
    _fields_ = [('kind', C.c_int32), ('rgb', C.c_uint8 * 3), ('npts', C.c_uint8), ('width', C.c_double), ('geom', C.c_double * RENDER_GEOM)]


class RenderCall(C.Structure):
    """include/d2d_render.h `d2d_render_call`."""
    _fields_ = [(n, C.c_void_p) for n in RENDER_CALL_POINTERS] + [(n, C.c_int32) for n in RENDER_CALL_INTS] + \
               [('view_range', C.c_double), ('star', C.c_double * 20)]


class RasterCall(C.Structure):
    """include/d2d_render_hooks.h `d2d_render_raster_call`."""
    _fields_ = [(n, C.c_void_p) for n in RASTER_CALL_POINTERS] + [(n, C.c_int32) for n in RASTER_CALL_INTS]


def bind_render(lib):
    """argtypes / restypes of include/d2d_render.h and include/d2d_render_hooks.h on a loaded CDLL."""
    P = C.POINTER
    sig = {
        'version': (C.c_int, []),
        'last_error': (C.c_char_p, []),
        'list': (C.c_int, [P(Cfg), P(State), P(RenderCall), C.c_void_p]),
        'frame': (C.c_int, [P(Cfg), P(State), P(RenderCall), C.c_void_p]),
        'raster': (C.c_int, [P(RasterCall), C.c_void_p]),
    }
    return _bind(lib, 'd2d_render_', sig)


# ---- include/d2d_capture.h: the terminal frames of streamed episodes (additions to csrc/render/libd2d_render.so) ----
RENDER_SKIPPED = 3
CAPTURE_KIND_NAMES = ('static', 'dynamic', 'dead_lock', 'freezing', 'goal', 'other')     # D2D_CAPTURE_* 1 .. 6, in the rule's order
CAPTURE_KINDS = len(CAPTURE_KIND_NAMES)
CAPTURE_META_F, CAPTURE_COUNTS = 4, 3
CAPTURE_M_EPISODE, CAPTURE_M_KIND, CAPTURE_M_STEPS, CAPTURE_M_SLOT = range(4)
CAPTURE_ENTRY_POINTS = ('capture_select', 'render_list_sel', 'render_frame_sel')


def bind_capture(lib):
    """argtypes / restypes of include/d2d_capture.h on the loaded libd2d_render.so: additions to that library, looked up as optional
    symbols (a build without them binds nothing here, and its version is the same)."""
    P, V, I = C.POINTER, C.c_void_p, C.c_int32
    sig = {
        'capture_select': (C.c_int, [P(Cfg), P(State), V, C.c_uint32, I, C.c_int64, V, V, V, V, V, V]),
        'render_list_sel': (C.c_int, [P(Cfg), P(State), P(RenderCall), V]),
        'render_frame_sel': (C.c_int, [P(Cfg), P(State), P(RenderCall), V, C.c_int64, V]),
    }
    return _bind(lib, 'd2d_', sig, CAPTURE_ENTRY_POINTS)
