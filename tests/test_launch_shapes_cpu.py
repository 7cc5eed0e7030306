"""What the host side of the HIP library answers without a GPU, against a recording (tests/golden/launch_shapes.json, written by
tests/golden/make_launch_shapes.py from the library as it was before its host dispatch was folded into pick_launch()):
d2d_launch_shape of a table of configurations -- the one description of a launch the tests and bench.py trust -- and every refusal
of the entry points, return code and d2d_last_error() text.  Every refusal row returns before any launch; pointers are dummies,
nothing is dereferenced."""
import ctypes as C
import itertools
import json
import os

import pytest

import closed_loop_cases as CL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_shapes.json')
NS = (0, 1, 16, 17, 40, 41, 64, 65, 128, 129, 172)
# default geometry, a row-major map of another size, a tiled map whose sides are not multiples of 16
GEOMETRIES = dict(default=({}, 0),
                  rowmajor=(dict(map_size=[600, 450], drone_view_range=120, drone_view_depth=60), 0),
                  tiled=(dict(map_size=[530, 470], drone_view_range=120, drone_view_depth=60), 16))
GAZES = ('GAZE_NONE', 'GAZE_OXFORD', 'GAZE_LOOKAHEAD', 'GAZE_LOOKGOAL', 'GAZE_OWL')
_BASE = dict(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
             map_id=1)


def _cfg_plan(pkg, N, B=3, tile=0, nomove=False, gaze='GAZE_OXFORD', primitive=True, launch_args=True, **kw):
    """d2d_cfg and d2d_plan (scalars only; launch_args is a dummy, nothing is dereferenced) of B envs with N agents"""
    from drone2d_amd import _abi as A, host_init, device_plugins
    p = pkg.with_defaults(pkg.Params(**dict(_BASE, **kw)))
    cfg = host_init.derive_cfg(p, B=B, N=N, T=1, planner_mode=A.PLANNER_NOMOVE if nomove else A.PLANNER_EXTERNAL, kf_enabled=True,
                               grid_tile=tile)
    sc, _ = device_plugins.build_tables(p, cfg, need_acos=False)
    plan = A.Plan()
    for k, v in sc.items():
        setattr(plan, k, v)
    plan.planner, plan.gaze = A.PLAN_PRIMITIVE if primitive else A.PLAN_NONE, getattr(A, gaze)
    plan.launch_args = 1 if launch_args else None
    return cfg, plan


def shape_table(pkg):
    """name -> (cfg, plan)"""
    rows = {}
    for c in CL.CASES:
        rows['case ' + CL.case_id(c)] = CL.cfg_and_plan(pkg, c)
    # tests/test_abi.py test_bench_workload_keeps_four_workgroups_per_cu
    rows['bench config2'] = _cfg_plan(pkg, 10, B=4096)
    rows['bench config3'] = _cfg_plan(pkg, 172, B=16)
    rows['bench config4'] = _cfg_plan(pkg, 24, B=16)
    rows['bench config5'] = _cfg_plan(pkg, 100, B=16, nomove=True, planner='NoMove', agent_number=100, agent_max_speed=40,
                                      map_size=[6400, 6400], init_pos=[3200, 3200], target_list=[[6000, 6000]])
    for (g, (kw, tile)), n in itertools.product(GEOMETRIES.items(), NS):
        rows[f'{g} N={n}'] = _cfg_plan(pkg, n, tile=tile, **kw)
    for n in (10, 17, 41):
        rows[f'var_cam N={n}'] = _cfg_plan(pkg, n, var_cam=2)
    # a single wave above 64 KB; a view no workgroup holds (wpb == 0)
    rows['1400 agents 1000x1000'] = _cfg_plan(pkg, 1400, map_size=[1000, 1000])
    rows['view depth 2100'] = _cfg_plan(pkg, 10, map_size=[3000, 3000], drone_view_depth=2100)
    for g in ('default', 'rowmajor'):
        kw, tile = GEOMETRIES[g]
        for gaze, prim, la, nomove in itertools.product(GAZES, (True, False), (True, False), (False, True)):
            name = f"{g} {gaze} planner={'on' if prim else 'off'} launch_args={'set' if la else 'null'} {'nomove' if nomove else 'external'}"
            rows[name] = _cfg_plan(pkg, 10, tile=tile, gaze=gaze, primitive=prim, launch_args=la, nomove=nomove, **kw)
    return rows


def record_shapes(pkg):
    from drone2d_amd import _lib
    return {name: dict(step=list(_lib.launch_shape(cfg)), closed=list(_lib.launch_shape(cfg, plan)), path=CL.closed_loop_path(cfg, plan))
            for name, (cfg, plan) in shape_table(pkg).items()}


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _good(pkg, gaze='GAZE_OXFORD', primitive=True, **kw):
    """A cfg / state / plan / snapshot every check accepts: all pointers are the dummy 1"""
    A = pkg._abi
    cfg, plan = _cfg_plan(pkg, 10, B=4, gaze=gaze, primitive=primitive, **kw)
    st, init = A.State(), A.State()
    for name, _ in A.State._fields_:
        setattr(st, name, 1)
        setattr(init, name, 1)
    for name in A.PLAN_TABLES + A.PLAN_STATE:
        setattr(plan, name, 1)
    return cfg, st, plan, init


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def refusal_table(pkg):
    """(entry point, defect) -> a call that returns the entry point's return code"""
    from drone2d_amd import _lib
    A = pkg._abi
    _, fn = _lib.load_library()
    R = C.byref
    rows = {}

    def add(entry, defect, call, gaze='GAZE_OXFORD', primitive=True, **change):
        """`change`: 'cfg' / 'st' / 'plan' / 'init' -> fields to set on the good structs before call(cfg, st, plan, init)"""
        def run():
            cfg, st, plan, init = _good(pkg, gaze=gaze, primitive=primitive)
            for which, obj in (('cfg', cfg), ('st', st), ('plan', plan), ('init', init)):
                _set(obj, **change.get(which, {}))
            return call(cfg, st, plan, init)
        assert (entry, defect) not in rows
        rows[entry, defect] = run

    step = lambda c, s, p, i: fn['step'](R(c), R(s), None)
    # check(), through d2d_step
    add('step', 'null cfg', lambda c, s, p, i: fn['step'](None, R(s), None))
    add('step', 'null state', lambda c, s, p, i: fn['step'](R(c), None, None))
    add('step', 'abi version', step, cfg=dict(abi_version=A.D2D_ABI_VERSION + 1))
    add('step', 'B < 0', step, cfg=dict(B=-1))
    add('step', 'even L', step, cfg=dict(L=32))
    add('step', 'noise_row0 past the rows', step, cfg=dict(noise_rows=4, noise_row0=4))
    add('step', 'grid_tile 8', step, cfg=dict(grid_tile=8))
    add('step', 'W 40000', step, cfg=dict(W=40000))
    add('step', 'scale 1', step, cfg=dict(scale=1.0))
    add('step', 'scale 2.5', step, cfg=dict(scale=2.5))
    add('step', 'depth 0', step, cfg=dict(depth=0.0))
    add('step', 'kf without buffers', step, st=dict(kf=None))
    add('step', 'var_cam without noise', step, cfg=dict(sigma=2.0), st=dict(noise=None, rng=None))
    add('step', 'rng without rng_draws', step, st=dict(rng_draws=None))
    add('step', 'null flags', step, st=dict(flags=None))
    add('step', 'view too deep', step, cfg=dict(depth=21000.0, L=8401, W=3000, H=3000, W_px=30000.0, H_px=30000.0))
    # launch_stages
    add('step', 'null action', step, st=dict(action=None))
    add('step', 'external planner without wp', step, st=dict(wp=None))
    add('perceive', 'null action is fine, B == 0', lambda c, s, p, i: fn['perceive'](R(c), R(s), None), cfg=dict(B=0), st=dict(action=None))
    add('step', 'B == 0', step, cfg=dict(B=0))
    add('act', 'B == 0', lambda c, s, p, i: fn['act'](R(c), R(s), None), cfg=dict(B=0))
    add('run_stages', 'B == 0', lambda c, s, p, i: fn['run_stages'](R(c), R(s), A.ST_RAYCAST, None), cfg=dict(B=0))
    # reset_launch
    reset = lambda c, s, p, i: fn['reset'](R(c), R(s), R(i), None, None)
    add('reset', 'null snapshot', lambda c, s, p, i: fn['reset'](R(c), R(s), None, None, None))
    add('reset', 'snapshot without active', reset, init=dict(active=None))
    add('reset', 'bad state first', reset, st=dict(hit=None))
    add('reset', 'B == 0', reset, cfg=dict(B=0))
    # d2d_rollout
    roll = lambda n, actions=1: (lambda c, s, p, i: fn['rollout'](R(c), R(s), n, actions, None, None, None, None))
    add('rollout', 'null actions', roll(4, None))
    add('rollout', 'nsteps < 0', roll(-1))
    add('rollout', 'bad state first', roll(4), st=dict(gt=None))
    add('rollout', 'nsteps == 0', roll(0))
    add('rollout', 'B == 0', roll(4), cfg=dict(B=0))
    add('rollout', 'external planner without wp', roll(4), st=dict(wp=None))
    # plan_check, through d2d_plan_stage / d2d_gaze_stage / d2d_closed_loop
    ps = lambda c, s, p, i: fn['plan_stage'](R(c), R(s), R(p), None)
    gs = lambda c, s, p, i: fn['gaze_stage'](R(c), R(s), R(p), None)
    add('plan_stage', 'bad state first', ps, st=dict(drone=None))
    add('plan_stage', 'null plan', lambda c, s, p, i: fn['plan_stage'](R(c), R(s), None, None))
    add('gaze_stage', 'null plan', lambda c, s, p, i: fn['gaze_stage'](R(c), R(s), None, None))
    add('gaze_stage', 'gaze 4', gs, plan=dict(gaze=4))
    add('plan_stage', 'null traj', ps, plan=dict(traj=None))
    add('gaze_stage', 'Oxford without kf', gs, primitive=False, cfg=dict(kf_enabled=0))
    add('gaze_stage', 'LookAhead null action', gs, gaze='GAZE_LOOKAHEAD', st=dict(action=None))
    add('gaze_stage', 'LookAhead yaw_rate_max 0', gs, gaze='GAZE_LOOKAHEAD', plan=dict(yaw_rate_max=0.0))
    add('gaze_stage', 'LookGoal without traj', gs, gaze='GAZE_LOOKGOAL', primitive=False, plan=dict(traj_hdr=None))
    add('gaze_stage', 'LookGoal traj_cap 0', gs, gaze='GAZE_LOOKGOAL', primitive=False, plan=dict(traj_cap=0))
    add('gaze_stage', 'Owl null action', gs, gaze='GAZE_OWL', st=dict(action=None))
    add('gaze_stage', 'Owl yaw_rate_max 0', gs, gaze='GAZE_OWL', plan=dict(yaw_rate_max=0.0))
    add('gaze_stage', 'Owl without owl_tab', gs, gaze='GAZE_OWL', plan=dict(owl_tab=None))
    add('gaze_stage', 'Owl without kf', gs, gaze='GAZE_OWL', primitive=False, cfg=dict(kf_enabled=0))
    add('plan_stage', 'null hash', ps, plan=dict(hash=None))
    add('plan_stage', 'hash_cap not a power of two', ps, plan=dict(hash_cap=3 << 20))
    add('plan_stage', 'hash_cap <= node_cap', ps, plan=dict(hash_cap=1024))
    add('plan_stage', 'nu 0', ps, plan=dict(nu=0))
    add('plan_stage', 'traj_cap < n_ts', ps, plan=dict(traj_cap=3))
    add('plan_stage', 'without wp_valid', ps, st=dict(wp_valid=None))
    add('plan_stage', 'vmax_sq 1600', ps, plan=dict(vmax_sq=1600.0))
    add('plan_stage', 'goal_sq 99', ps, plan=dict(goal_sq=99.0))
    add('plan_stage', 'planner tables above the LDS', ps, plan=dict(nu=200))
    add('gaze_stage', 'null yaw_space', gs, plan=dict(yaw_space=None))
    add('gaze_stage', 'Oxford null action', gs, st=dict(action=None))
    add('gaze_stage', 'n_yaw 8', gs, plan=dict(n_yaw=8))
    add('gaze_stage', 'pw_nprog', gs, plan=dict(pw_nprog=7))
    add('gaze_stage', 'dense plan above the LDS', gs, cfg=dict(depth=140.0), plan=dict(pw_nleaf=20000, pw_nprog=39999))
    add('gaze_stage', '2^24 cells', gs, primitive=False, cfg=dict(W=4096, H=4096, W_px=40960.0, H_px=40960.0))
    add('gaze_stage', 'view depth 300', gs, primitive=False, cfg=dict(depth=300.0, L=121))
    add('gaze_stage', 'tobs_tab short', gs, plan=dict(tobs_len=100))
    add('gaze_stage', 'B == 0', gs, cfg=dict(B=0))
    add('plan_stage', 'B == 0', ps, cfg=dict(B=0))
    # d2d_closed_loop
    cl = lambda n, on_done=A.DONE_CONTINUE: (lambda c, s, p, i: fn['closed_loop'](R(c), R(s), R(p), n, on_done, R(i), None))
    add('closed_loop', 'bad plan first', cl(4), plan=dict(traj_hdr=None))
    add('closed_loop', 'nsteps < 0', cl(-1))
    add('closed_loop', 'on_done 3', cl(4, 3))
    add('closed_loop', 'on_done -1', cl(4, -1))
    add('closed_loop', 'reset without snapshot', lambda c, s, p, i: fn['closed_loop'](R(c), R(s), R(p), 4, A.DONE_RESET, None, None))
    add('closed_loop', 'reset with snapshot without gt', cl(4, A.DONE_RESET), init=dict(gt=None))
    add('closed_loop', 'B == 0', cl(4, A.DONE_RESET), cfg=dict(B=0))
    add('closed_loop', 'nsteps == 0', cl(0, A.DONE_FREEZE))
    add('closed_loop', 'nsteps == 0 per stage', cl(0), plan=dict(launch_args=None))
    # d2d_plan_reset
    pr = lambda c, s, p, i: fn['plan_reset'](R(c), R(p), None, 1, None)
    add('plan_reset', 'null cfg', lambda c, s, p, i: fn['plan_reset'](None, R(p), None, 1, None))
    add('plan_reset', 'null plan', lambda c, s, p, i: fn['plan_reset'](R(c), None, None, 1, None))
    add('plan_reset', 'abi version', pr, cfg=dict(abi_version=1))
    add('plan_reset', 'B == 0', pr, cfg=dict(B=0))
    # d2d_launch_shape
    out = (C.c_int32 * 4)()
    add('launch_shape', 'null cfg', lambda c, s, p, i: fn['launch_shape'](None, None, R(out)))
    add('launch_shape', 'null out', lambda c, s, p, i: fn['launch_shape'](R(c), None, None))
    add('launch_shape', 'abi version', lambda c, s, p, i: fn['launch_shape'](R(c), R(p), R(out)), cfg=dict(abi_version=0))
    # the array entry points
    for name, nptr in (('sincos_array', 3), ('tan_array', 2), ('atan2_array', 3), ('pow2_array', 2), ('log_array', 2)):
        f = fn[name]
        add(name, 'n < 0', lambda c, s, p, i, f=f, k=nptr: f(*([1] * k), -1, None))
        add(name, 'null out, n > 0', lambda c, s, p, i, f=f, k=nptr: f(*([1] * (k - 1)), None, 5, None))
        add(name, 'null in, n > 0', lambda c, s, p, i, f=f, k=nptr: f(None, *([1] * (k - 1)), 5, None))
        add(name, 'n == 0', lambda c, s, p, i, f=f, k=nptr: f(*([1] * k), 0, None))
        add(name, 'null pointers, n == 0', lambda c, s, p, i, f=f, k=nptr: f(*([None] * k), 0, None))
    add('rng_draw', 'null rng', lambda c, s, p, i: fn['rng_draw'](None, 1, 1, 4, 4, None))
    add('rng_draw', 'max_m < 0', lambda c, s, p, i: fn['rng_draw'](1, 1, 1, 4, -1, None))
    add('rng_draw', 'B == 0', lambda c, s, p, i: fn['rng_draw'](1, 1, 1, 0, 4, None))
    return rows, fn


def record_refusals(pkg):
    rows, fn = refusal_table(pkg)
    out = {}
    for (entry, defect), run in rows.items():
        rc = run()
        out[f'{entry}: {defect}'] = [rc, fn['last_error']().decode() if rc else '']
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_launch_shapes_are_the_recorded_ones(pkg, golden):
    got = record_shapes(pkg)
    assert sorted(got) == sorted(golden['shapes'])
    for name, row in got.items():
        assert row == golden['shapes'][name], name


def test_table_holds_what_it_is_for(golden):
    """The recording covers every kernel of the dispatch, every waves-per-workgroup answer, the single wave above 64 KB and the
    two reporting quirks (wpb 0 with LDS bytes from one wave never happens: bytes are 0 whenever wpb is)."""
    sh = golden['shapes']
    assert {r['path'] for r in sh.values()} >= set(CL.PATHS) | {'per_stage_gaze'}
    assert {r['step'][0] for r in sh.values()} == {0, 1, 2, 4}
    assert sh['1400 agents 1000x1000']['step'][0] == 1 and sh['1400 agents 1000x1000']['step'][1] > 64 * 1024
    assert sh['view depth 2100']['step'] == [0, 0, 0, 0] and sh['view depth 2100']['closed'][:3] == [0, 0, 0]
    for name, r in sh.items():
        assert (r['closed'][0] == 1) == (' launch_args=null' not in name and ' nomove' not in name
                                         and r['path'] not in ('per_stage_nomove', 'per_stage_primitive')
                                         and name != 'view depth 2100'), name


def test_refusals_are_the_recorded_ones(pkg, golden):
    got = record_refusals(pkg)
    assert sorted(got) == sorted(golden['refusals'])
    for name, row in got.items():
        assert row == golden['refusals'][name], name
    # every fail() text of the host code that is not a HIP error string is in the table
    src = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'gym-drone2d-activeperception_amd', 'csrc', 'd2d_hip.hip')).read()
    import re
    texts = {row[1] for row in got.values()}
    for code, lit in re.findall(r'fail\((-\d), ((?:\s*"(?:[^"\\]|\\.)*")+)\)', src):
        text = ''.join(re.findall(r'"((?:[^"\\]|\\.)*)"', lit))
        assert text in texts, (code, text)
