"""The launch paths of d2d_closed_loop and the case table that runs every one of them (test infrastructure, like replay.py and
oracle_lib.py): tests/test_gpu_closed_loop_paths.py runs the table against the oracle on the GPU, tests/test_closed_loop_paths_cpu.py
checks on every CPU run that each row takes its declared path and that the table covers every pairing below."""
import itertools

# csrc/d2d_hip.hip d2d_closed_loop: one persistent launch (k_closed<SPEC>) or one launch per stage per step
PATHS = ('k_closed<1>',          # default geometry, row-major grids, var_cam == 0, N <= 16
         'k_closed<2>',          # the same with 17 <= N <= 40
         'k_closed<3>',          # the same with N > 40
         'k_closed<0>',          # any other geometry (or var_cam != 0) on row-major grids
         'k_closed<4>',          # any other geometry on tiled grids (grid_tile = 16)
         'per_stage_nomove',     # planner_mode == D2D_PLANNER_NOMOVE: k_gaze + k_stages per step
         'per_stage_primitive')  # d2d_plan.launch_args == NULL: k_gaze, k_stages, k_plan, k_stages per step
GAZES = ('Oxford', 'LookAhead', 'LookGoal', 'constant')
ON_DONE = ('continue', 'reset', 'freeze')
NOISE_ROWS = 7          # rows of the [T, B, N, 2] noise tensor of the noise rows: a run wraps around them

# spec_default_matches (csrc/d2d_hip.hip): the literals the specialised kernels fold in
_DEFAULT_GEOMETRY = dict(W=50, H=50, R=50, L=33, dt=0.1, scale=10.0, W_px=500.0, H_px=500.0,
                         ray_off0=float.fromhex('-0x1.921fb54442d18p-1'), ray_dth=float.fromhex('0x1.015bf9217271ap-5'),
                         depth=80.0, drone_radius=10.0, yaw_rate=80.0, max_acc=40.0, max_steps=800.0, sigma=0.0, grid_tile=0)


def default_geometry(cfg):
    return all(getattr(cfg, k) == v for k, v in _DEFAULT_GEOMETRY.items())


def closed_loop_path(cfg, plan):
    """Which code path d2d_closed_loop takes for (cfg, plan), restated from its dispatch.  Needs the HIP library (launch_shape),
    not a GPU.  Raises if the restatement of the default geometry and the library's launch_shape disagree."""
    from drone2d_amd import _abi as A, _lib
    if cfg.planner_mode == A.PLANNER_NOMOVE:
        return 'per_stage_nomove'
    persistent = bool(plan.launch_args) and (plan.planner == A.PLAN_PRIMITIVE or plan.gaze != A.GAZE_NONE)
    if persistent and _lib.launch_shape(cfg, plan)[0] == 1:
        default = default_geometry(cfg)
        # launch_shape()[3]: the grids staged whole, which only SPEC 1 and 2 do (the default geometry with N <= 40)
        whole = _lib.launch_shape(cfg)[3] == 1
        assert whole == (default and cfg.N <= 40), ('default geometry restated wrongly', default, whole, cfg.N)
        if not default:
            return 'k_closed<4>' if cfg.grid_tile else 'k_closed<0>'
        return 'k_closed<1>' if cfg.N <= 16 else ('k_closed<2>' if cfg.N <= 40 else 'k_closed<3>')
    return 'per_stage_primitive' if plan.planner == A.PLAN_PRIMITIVE else 'per_stage_gaze'


def _row(path, gaze, on_done, B, T, chunks, layout='rowmajor', noise=False, zero_call=False, null_box=False, **kw):
    policy = {'constant': 'Rotating'}.get(gaze, gaze)
    if gaze not in GAZES:                                   # a constant policy by name
        policy, gaze = gaze, 'constant'
    return dict(path=path, gaze=gaze, policy=policy, on_done=on_done, B=B, T=T, chunks=chunks, layout=layout, noise=noise,
                zero_call=zero_call, null_box=null_box, kw=kw)


# the default geometry with the default max_flight_time (the specialised kernels need max_steps == 800): episodes end by goal
# (a near target, fast drones) or by collision (fast, large agents)
_NEAR = dict(init_pos=[60, 60], target_list=[[70, 200]], drone_max_speed=50)
_FAST = dict(agent_radius=15, agent_max_speed=60)
# another geometry (k_closed<0> / <4>): a short max_flight_time ends every episode that nothing else ends
_OTHER = dict(drone_view_range=120, drone_view_depth=60, max_flight_time=8)
# 2000 x 1600 px, pillars, fast agents: trajectories of many hundred waypoints, walked through their chunk boxes (traj_box)
_LONG = dict(agent_number=30, agent_radius=12, agent_max_speed=60, map_size=[2000, 1600], pillar_number=9, init_pos=[120, 120],
             target_list=[[1880, 1480], [120, 1480]], max_flight_time=10)

CASES = [
    # ---- k_closed<1>: N <= 16
    _row('k_closed<1>', 'Oxford', 'continue', 3, 80, [7], agent_number=12, map_id=301, **_NEAR, **_FAST),
    _row('k_closed<1>', 'LookAhead', 'reset', 1, 120, [1, 9], agent_number=16, map_id=302, **_NEAR, **_FAST),
    _row('k_closed<1>', 'LookGoal', 'freeze', 5, 80, [5, 12, 3], agent_number=10, map_id=303, pillar_number=4, **_NEAR, **_FAST),
    _row('k_closed<1>', 'Rotating', 'continue', 3, 70, [10, 1], zero_call=True, agent_number=8, map_id=304, **_NEAR, **_FAST),
    # ---- k_closed<2>: 17 <= N <= 40 (obstacle_map brings 14 agents of its own)
    _row('k_closed<2>', 'Oxford', 'reset', 3, 90, [9], agent_number=30, agent_radius=10, agent_max_speed=60, map_id=311, **_NEAR),
    _row('k_closed<2>', 'LookAhead', 'freeze', 3, 80, [4, 11], agent_number=10, map_id=312, static_map='maps/obstacle_map.npy',
         **_NEAR, **_FAST),
    _row('k_closed<2>', 'LookGoal', 'continue', 5, 60, [6], agent_number=40, agent_radius=8, agent_max_speed=60, map_id=313, **_NEAR),
    _row('k_closed<2>', 'NoControl', 'reset', 6, 80, [3, 13], agent_number=17, map_id=314, **_NEAR, **_FAST),
    # ---- k_closed<3>: N > 40
    _row('k_closed<3>', 'Oxford', 'freeze', 3, 60, [12, 5], agent_number=48, agent_radius=8, agent_max_speed=60, map_id=321, **_NEAR),
    _row('k_closed<3>', 'LookAhead', 'continue', 3, 60, [8], agent_number=41, agent_radius=8, agent_max_speed=60, map_id=322, **_NEAR),
    _row('k_closed<3>', 'LookGoal', 'reset', 3, 60, [7, 2], agent_number=10, map_id=323, static_map='maps/random_map_0.npy',
         agent_radius=5, agent_max_speed=60, init_pos=[250, 30], target_list=[[250, 160]], drone_max_speed=50),
    _row('k_closed<3>', 'Rotating', 'freeze', 3, 60, [15], agent_number=64, agent_radius=6, agent_max_speed=60, map_id=324, **_NEAR),
    # ---- k_closed<0>: any other geometry on row-major grids (var_cam != 0 included)
    _row('k_closed<0>', 'Oxford', 'continue', 3, 100, [7, 13], noise=True, var_cam=2, agent_number=20, agent_radius=12,
         agent_max_speed=30, map_id=331, map_size=[600, 450], init_pos=[300, 220], target_list=[[520, 380]], **_OTHER),
    _row('k_closed<0>', 'LookAhead', 'reset', 5, 90, [1, 6], agent_number=12, agent_radius=12, agent_max_speed=40, map_id=332,
         map_size=[700, 400], init_pos=[80, 80], target_list=[[600, 320]], drone_radius=15, **_OTHER),
    _row('k_closed<0>', 'LookGoal', 'freeze', 3, 90, [9], agent_number=14, agent_radius=10, agent_max_speed=30, map_id=333,
         map_size=[1000, 700], map_scale=20, init_pos=[100, 100], target_list=[[850, 600]], drone_max_speed=60,
         drone_view_range=120, max_flight_time=8),
    _row('k_closed<0>', 'Rotating', 'reset', 3, 80, [5, 11], noise=True, var_cam=2, agent_number=10, agent_radius=15,
         agent_max_speed=40, map_id=334, init_pos=[250, 250], target_list=[[250, 420]]),
    # ---- k_closed<4>: tiled grids whose sides are not multiples of 16 (partial edge tiles)
    _row('k_closed<4>', 'Oxford', 'reset', 3, 90, [6, 9], layout='tiled', agent_number=14, agent_radius=12, agent_max_speed=40,
         map_id=341, map_size=[530, 470], init_pos=[450, 60], target_list=[[80, 400]], **_OTHER),
    _row('k_closed<4>', 'LookAhead', 'freeze', 3, 90, [11], layout='tiled', agent_number=12, agent_radius=12, agent_max_speed=40,
         map_id=342, map_size=[1060, 940], map_scale=20, init_pos=[120, 120], target_list=[[900, 800]], drone_max_speed=60,
         max_flight_time=8),
    _row('k_closed<4>', 'LookGoal', 'continue', 3, 90, [1, 14], layout='tiled', noise=True, var_cam=2, agent_number=24,
         agent_radius=10, agent_max_speed=40, map_id=343, map_size=[470, 530], init_pos=[60, 60], target_list=[[400, 470]],
         **_OTHER),
    _row('k_closed<4>', 'NoControl', 'freeze', 5, 80, [8], layout='tiled', agent_number=10, agent_radius=15, agent_max_speed=50,
         map_id=344, map_size=[690, 330], init_pos=[345, 165], target_list=[[640, 300]], max_flight_time=6),
    # ---- one launch per stage, NoMove (reset and freeze inside k_gaze, D2D_ST_SKIP_DONE)
    _row('per_stage_nomove', 'Oxford', 'freeze', 5, 80, [7, 3], noise=True, var_cam=2, agent_number=20, agent_radius=15,
         agent_max_speed=60, map_id=351, init_pos=[250, 250]),
    _row('per_stage_nomove', 'LookAhead', 'freeze', 3, 80, [1, 10], agent_number=16, agent_radius=15, agent_max_speed=60,
         map_id=352, map_size=[600, 400], init_pos=[300, 200], max_flight_time=6),
    _row('per_stage_nomove', 'LookGoal', 'reset', 3, 80, [9, 4], layout='tiled', agent_number=12, agent_radius=15,
         agent_max_speed=60, map_id=353, map_size=[530, 470], init_pos=[260, 230], max_flight_time=5),
    _row('per_stage_nomove', 'Rotating', 'continue', 1, 90, [13], map_scale=20, agent_number=10, agent_radius=15,
         agent_max_speed=60, map_id=354, map_size=[800, 600], init_pos=[400, 300], max_flight_time=4),
    # ---- one launch per stage, Primitive (launch_args = NULL)
    _row('per_stage_primitive', 'Oxford', 'continue', 3, 80, [5, 8], noise=True, var_cam=2, agent_number=24, agent_radius=12,
         agent_max_speed=40, map_id=361, init_pos=[250, 250], target_list=[[250, 420]], max_flight_time=6),
    _row('per_stage_primitive', 'LookAhead', 'reset', 3, 90, [1, 12], agent_number=10, map_id=362, **_NEAR, **_FAST),
    _row('per_stage_primitive', 'LookGoal', 'freeze', 3, 90, [10, 7], layout='tiled', agent_number=12, agent_radius=12,
         agent_max_speed=40, map_id=363, map_size=[530, 470], init_pos=[450, 60], target_list=[[80, 400]], **_OTHER),
    _row('per_stage_primitive', 'NoControl', 'continue', 6, 70, [7, 4], noise=True, var_cam=2, agent_number=12, agent_radius=15,
         agent_max_speed=50, map_id=364, map_size=[600, 450], init_pos=[300, 220], target_list=[[540, 400]], max_flight_time=5),
    # ---- d2d_plan.traj_box = NULL (every walk visits every chunk): the long trajectories, persistent and per stage
    _row('k_closed<0>', 'Oxford', 'reset', 3, 120, [16, 7], null_box=True, map_id=371, **_LONG),
    _row('per_stage_primitive', 'Oxford', 'freeze', 3, 120, [16, 7], null_box=True, map_id=372, **_LONG),
]


def case_id(c):
    p = c['path'].replace('k_closed<', 'closed').replace('>', '').replace('per_stage_', 'stage_')
    return f"{p}-{c['policy']}-{c['on_done']}" + ('-nullbox' if c['null_box'] else '')


def planner_of(c):
    return 'NoMove' if c['path'] == 'per_stage_nomove' else 'Primitive'


def params_of(pkg, c):
    return pkg.Params(planner=planner_of(c), gaze_method=c['policy'], **c['kw'])


def chunk_sizes(c):
    """The row's T steps cut into calls of its (cycled) chunk sizes"""
    out, left = [], c['T']
    for n in itertools.cycle(c['chunks']):
        if left <= 0:
            return out
        out.append(min(n, left))
        left -= out[-1]


def cfg_and_plan(pkg, c, device='cpu'):
    """The d2d_cfg and d2d_plan a VecDrone2DEnv builds for row `c` (host_init.derive_cfg + PluginState), without a backend"""
    from drone2d_amd import _abi as A, host_init
    from drone2d_amd.device_plugins import PluginState
    p = pkg.with_defaults(params_of(pkg, c))
    w = host_init.init_world(p)
    nomove = planner_of(c) == 'NoMove'
    cfg = host_init.derive_cfg(p, B=c['B'], N=w['N'], T=w['T'], planner_mode=A.PLANNER_NOMOVE if nomove else A.PLANNER_EXTERNAL,
                               kf_enabled=True, grid_tile=16 if c['layout'] == 'tiled' else 0)
    ps = PluginState(p, cfg, device, [w['tracker_radius']] * c['B'], planner=planner_of(c), gaze=c['policy'])
    plan = ps.struct()
    adjust_plan(c, plan)
    return cfg, plan


def adjust_plan(c, plan):
    """What a row changes in the d2d_plan the env built: the forced per-stage path, the missing chunk boxes"""
    if c['path'] == 'per_stage_primitive':
        plan.launch_args = None
    if c['null_box']:
        plan.traj_box = None
