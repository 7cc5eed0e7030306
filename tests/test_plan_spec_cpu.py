"""csrc/d2d_plan_spec.h compiled for the host: which (d2d_cfg, d2d_plan) the host dispatch of d2d_closed_loop hands to the persistent
kernel with the plugins' default parameters folded in (k_closed<1, true>), and what that kernel writes over its copy of the plan.
The structs come from the package's own constructors (host_init.derive_cfg, device_plugins.PluginState), so a change of how they are
filled that the literals do not follow shows here: the headline workload would silently leave the folded kernel."""
import ctypes as C
import math

import pytest

import host_build
from drone2d_amd import _abi as A

# the headline workload (bench.py's config 2, the README's command): Params' defaults with 10 agents of radius 15
HEADLINE = dict(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
                map_id=1)
# the scalars plan_default_matches compares and plan_default_apply writes
MATCHED_INT = ('planner', 'gaze', 'nu', 'n_sample', 'n_ts', 'max_itr', 'n_yaw')
MATCHED_F64 = ('horizon', 'vmax', 'safe_dist', 'goal_tol', 'agent_radius', 'half_fov', 'yaw_rate_max', 'vmax_sq', 'goal_sq')
# what stays a run-time value: a change there must not leave the folded kernel
FREE_INT = ('traj_cap', 'node_cap', 'hash_cap', 'pw_nleaf', 'pw_nprog', 'tobs_len', 'pw_ntree')


@pytest.fixture(scope='module')
def spec(tmp_path_factory):
    lib = host_build.shared('plan_spec_host.cpp', tmp_path_factory.mktemp('planspec'), 'libplanspec.so')
    V = C.c_void_p
    lib.plan_spec_geometry_matches.argtypes = [V]
    lib.plan_spec_geometry_apply.argtypes = [V]
    lib.plan_spec_matches.argtypes = [V, V]
    lib.plan_spec_apply.argtypes = [V]
    return lib


def build(pkg, gaze='Oxford', planner='Primitive', **kw):
    """(cfg, plan, keep-alive) as a VecDrone2DEnv builds them for Params(**HEADLINE, **kw), without a backend"""
    from drone2d_amd import host_init
    from drone2d_amd.device_plugins import PluginState
    p = pkg.with_defaults(pkg.Params(**dict(HEADLINE, gaze_method=gaze, **kw)))
    w = host_init.init_world(p)
    cfg = host_init.derive_cfg(p, B=2, N=w['N'], T=w['T'], planner_mode=A.PLANNER_EXTERNAL, kf_enabled=True)
    ps = PluginState(p, cfg, 'cpu', [w['tracker_radius']] * 2, planner=planner, gaze=gaze)
    return cfg, ps.struct(), ps


def matches(spec, cfg, plan):
    return bool(spec.plan_spec_matches(C.addressof(cfg), C.addressof(plan)))


def test_the_structs_are_the_abi_ones(spec):
    assert spec.plan_spec_sizeof_cfg() == C.sizeof(A.Cfg) and spec.plan_spec_sizeof_plan() == C.sizeof(A.Plan)


def test_headline_plan_matches(pkg, spec):
    cfg, plan, _keep = build(pkg)
    assert cfg.N == 10 and matches(spec, cfg, plan)
    assert plan.half_fov == math.radians(45.0) and plan.vmax_sq != 0.0 and plan.goal_sq != 0.0
    assert math.sqrt(plan.vmax_sq) < 40.0 <= math.sqrt(math.nextafter(plan.vmax_sq, math.inf))
    assert math.sqrt(plan.goal_sq) <= 10.0 < math.sqrt(math.nextafter(plan.goal_sq, math.inf))
    cfg16, plan16, _keep16 = build(pkg, agent_number=16)
    assert cfg16.N == 16 and matches(spec, cfg16, plan16)          # the whole range of SPEC 1


@pytest.mark.parametrize('kw', [dict(drone_max_speed=30), dict(drone_view_range=60), dict(drone_max_yaw_speed=60), dict(agent_radius=10),
                                dict(agent_number=17), dict(drone_max_acceleration=30), dict(dt=0.05), dict(var_cam=1)],
                         ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_one_parameter_away_does_not_match(pkg, spec, kw):
    cfg, plan, _keep = build(pkg, **kw)
    assert not matches(spec, cfg, plan)


def test_other_plugins_do_not_match(pkg, spec):
    for gaze in ('LookAhead', 'LookGoal', 'Owl', 'NoControl'):
        cfg, plan, _keep = build(pkg, gaze=gaze)
        assert plan.gaze != A.GAZE_OXFORD and not matches(spec, cfg, plan), gaze
    cfg, plan, _keep = build(pkg, planner='NoMove')
    assert plan.planner == A.PLAN_NONE and not matches(spec, cfg, plan)


def test_every_matched_scalar_is_compared(pkg, spec):
    """One field of the matching plan changed at a time, by the smallest step there is"""
    cfg, plan, _keep = build(pkg)
    for name in MATCHED_INT:
        for d in (-1, 1):
            old = getattr(plan, name)
            setattr(plan, name, old + d)
            assert not matches(spec, cfg, plan), (name, d)
            setattr(plan, name, old)
    for name in MATCHED_F64:
        old = getattr(plan, name)
        for v in (math.nextafter(old, -math.inf), math.nextafter(old, math.inf), 0.0, -old, math.nan):
            setattr(plan, name, v)
            assert not matches(spec, cfg, plan), (name, v)
        setattr(plan, name, old)
    assert matches(spec, cfg, plan)
    # the "find it at every search" form of the two thresholds is another plan
    for name in ('vmax_sq', 'goal_sq'):
        old = getattr(plan, name)
        setattr(plan, name, 0.0)
        assert not matches(spec, cfg, plan), name
        setattr(plan, name, old)


def test_capacities_pointers_and_the_arccos_window_stay_free(pkg, spec):
    cfg, plan, _keep = build(pkg)
    for name in FREE_INT:
        setattr(plan, name, getattr(plan, name) + 8)
    plan.acos_key_lo += 3
    plan.acos_mask ^= 0xff
    for name in A.PLAN_TABLES + A.PLAN_STATE:
        setattr(plan, name, None)
    cfg.B, cfg.T, cfg.noise_rows, cfg.kf_enabled = 4096, 3, 7, 0
    assert matches(spec, cfg, plan)


def test_geometry_gates_the_plan(pkg, spec):
    cfg, plan, _keep = build(pkg)
    assert spec.plan_spec_geometry_matches(C.addressof(cfg))
    for name, v in (('W', 51), ('grid_tile', 16), ('sigma', 1.0), ('depth', 60.0), ('N', 17), ('N', 41)):
        old = getattr(cfg, name)
        setattr(cfg, name, v)
        assert not matches(spec, cfg, plan), name
        setattr(cfg, name, old)
    assert matches(spec, cfg, plan)


def test_apply_writes_the_matched_values(pkg, spec):
    """The literals ARE the matched values: a matching plan (and a default geometry) passes through apply byte for byte; any plan comes
    out with the matched scalars of the headline's and everything else untouched"""
    cfg, plan, _keep = build(pkg)
    before = bytes(plan)
    spec.plan_spec_apply(C.addressof(plan))
    assert bytes(plan) == before
    cfg_before = bytes(cfg)
    spec.plan_spec_geometry_apply(C.addressof(cfg))
    assert bytes(cfg) == cfg_before
    cfg2, other, _keep2 = build(pkg, gaze='LookAhead', drone_max_speed=30, drone_view_range=60, drone_max_yaw_speed=60, agent_radius=10)
    assert not matches(spec, cfg2, other)
    untouched = {n: getattr(other, n) for n, _ in A.Plan._fields_ if n not in MATCHED_INT + MATCHED_F64}
    spec.plan_spec_apply(C.addressof(other))
    for name in MATCHED_INT + MATCHED_F64:
        a, b = getattr(other, name), getattr(plan, name)
        assert (a == b) and (not isinstance(a, float) or a.hex() == b.hex()), name
    assert untouched == {n: getattr(other, n) for n in untouched}
