"""LookAhead / LookGoal gaze stages without a GPU: the C ABI additions, the launch geometry, the plan checks of the HIP library
(dummy pointers: every call is refused before a launch) and the refusal on a backend without the stages."""
import ctypes as C
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_constants_and_hook_match_the_bindings(pkg):
    from drone2d_amd import _lib
    A = pkg._abi
    d = dict(re.findall(r'#define\s+(D2D_\w+)\s+(\d+)\b', open(os.path.join(ROOT, 'include', 'd2d.h')).read()))
    assert (int(d['D2D_GAZE_LOOKAHEAD']), int(d['D2D_GAZE_LOOKGOAL'])) == (A.GAZE_LOOKAHEAD, A.GAZE_LOOKGOAL) == (2, 3)
    assert int(d['D2D_ABI_VERSION']) == A.D2D_ABI_VERSION == 8            # additive: no version bump, no struct change
    hooks = open(os.path.join(ROOT, 'include', 'd2d_hooks.h')).read()
    assert re.findall(r'^int\s+(d2d_\w+)\s*\(', hooks, flags=re.M) == ['d2d_' + n for n in A.HIP_ONLY_ENTRY_POINTS]
    assert 'atan2_array' in A.OPTIONAL and 'atan2_array' not in A.ENTRY_POINTS   # the oracle mirrors ENTRY_POINTS only
    lib, fn = _lib.load_library()
    assert fn['atan2_array'](None, None, None, 5, None) == -1 and fn['atan2_array'](None, None, None, 0, None) == 0
    assert _lib.HipBackend.supports_device_heading_gaze


def _plan(pkg, B):
    from drone2d_amd import host_init, device_plugins
    A = pkg._abi
    p = pkg.with_defaults(pkg.Params(planner='Primitive', gaze_method='LookAhead', agent_number=10, agent_radius=15,
                                     agent_max_speed=20, drone_max_speed=40, map_id=1))
    cfg = host_init.derive_cfg(p, B=B, N=10, T=1, planner_mode=A.PLANNER_EXTERNAL, kf_enabled=True)
    plan = A.Plan()
    for k, v in device_plugins.build_tables(p, cfg, need_acos=False)[0].items():
        setattr(plan, k, v)
    return cfg, plan


@pytest.mark.parametrize('planner', [1, 0])
def test_launch_shape_of_the_new_gaze_values_is_that_of_no_gaze(pkg, planner):
    """LookAhead / LookGoal use no LDS: the persistent launch keeps exactly the geometry of D2D_GAZE_NONE."""
    from drone2d_amd import _lib
    A = pkg._abi
    cfg, plan = _plan(pkg, 4096)
    plan.planner, plan.launch_args = planner, 1          # any non-null launch_args: the persistent path (nothing is dereferenced)
    shapes = []
    for g in (A.GAZE_NONE, A.GAZE_LOOKAHEAD, A.GAZE_LOOKGOAL):
        plan.gaze = g
        shapes.append(_lib.launch_shape(cfg, plan))
    assert shapes[0] == shapes[1] == shapes[2], shapes


def test_bad_heading_gaze_plans_are_refused_without_gpu(pkg):
    """Unknown gaze values (any value but 1 used to be a silent no-op), a yaw rate limit that is not > 0, LookGoal without the
    trajectory buffers and a missing action buffer are refused before any launch."""
    from drone2d_amd import _lib
    A = pkg._abi
    _, fn = _lib.load_library()
    cfg, plan = _plan(pkg, 4)
    st = A.State()
    for name, _ in A.State._fields_:
        setattr(st, name, 1)
    for name in A.PLAN_TABLES + A.PLAN_STATE:
        setattr(plan, name, 1)
    plan.planner = A.PLAN_NONE

    def refused(what):
        return fn['gaze_stage'](C.byref(cfg), C.byref(st), C.byref(plan), None) == -1 and what in fn['last_error']().decode()
    for g in (4, 7, -1):
        plan.gaze = g
        assert refused('unknown gaze'), g
        assert fn['closed_loop'](C.byref(cfg), C.byref(st), C.byref(plan), 1, 0, None, None) == -1
    for g in (A.GAZE_LOOKAHEAD, A.GAZE_LOOKGOAL):
        plan.gaze = g
        for bad in (0.0, -80.0, math.nan):
            plan.yaw_rate_max = bad
            assert refused('yaw_rate_max'), (g, bad)
        plan.yaw_rate_max = 80.0
    for field in ('traj', 'traj_hdr'):
        setattr(plan, field, None)
        assert refused('trajectory'), field
        setattr(plan, field, 1)
    st.action = None
    assert refused('action')


def test_heading_gaze_is_refused_on_a_backend_without_the_stage(pkg, oracle):
    """The CPU oracle runs only Oxford's gaze stage: a device LookAhead / LookGoal there is an error, not a silent no-op."""
    from drone2d_amd import vec_env, runner
    for gaze in ('LookAhead', 'LookGoal'):
        p = pkg.Params(planner='Primitive', gaze_method=gaze, agent_number=4, agent_radius=10, map_id=1)
        with pytest.raises(NotImplementedError, match='LookAhead / LookGoal'):
            vec_env.VecDrone2DEnv(p, 2, backend=oracle, planner='Primitive', device_plugins=True, gaze=gaze)
    with pytest.raises(NotImplementedError, match='LookGoal'):
        runner.ExperimentBatch(p, 2, device='cpu', backend=oracle)
