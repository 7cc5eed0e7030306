"""The Owl gaze stage without a GPU: the C ABI additions, the launch geometry, the plan checks of the HIP library (dummy pointers:
every call is refused before a launch), the refusal on a backend without the stage, the host table against the reference's
expressions, and the scalar model of tests/owl_model.py -- the device stage's specification -- against the package's host policy
`gaze.Owl` (numpy, as the reference) on every decision of the golden Owl episodes."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import owl_model as OM
from replay import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (fixture, case): the two Owl episodes of host_gaze_rows and the six of owl_episodes
EPISODES = [('host_gaze_rows', 3), ('host_gaze_rows', 4)] + [('owl_episodes', i) for i in range(6)]


def episode_id(ep):
    return f'{ep[0]}-r{ep[1]}'


def test_header_constants_and_hook_match_the_bindings(pkg):
    from drone2d_amd import _lib
    A = pkg._abi
    d = dict(re.findall(r'#define\s+(D2D_\w+)\s+(\d+)\b', open(os.path.join(ROOT, 'include', 'd2d.h')).read()))
    assert int(d['D2D_GAZE_OWL']) == A.GAZE_OWL == 5
    assert int(d['D2D_ABI_VERSION']) == A.D2D_ABI_VERSION == 8            # additive: no version bump
    for name in ('NRATE', 'NDIR', 'T_RATE', 'T_RATE08', 'T_TURN', 'T_ACT', 'T_DIR', 'T_FOV', 'T_DEPTH', 'T_HOLD', 'TAB_LEN',
                 'STATE_F', 'S_RATE', 'S_LEFT'):
        assert int(d['D2D_OWL_' + name]) == getattr(A, 'OWL_' + name), name
    assert A.OWL_T_DIR + 2 * A.OWL_NDIR <= A.OWL_T_FOV < A.OWL_T_HOLD < A.OWL_TAB_LEN and A.OWL_NDIR <= A.OWL_S_RATE < A.OWL_S_LEFT < A.OWL_STATE_F
    assert A.PLAN_TABLES[-1] == 'owl_tab' and A.PLAN_STATE[-1] == 'owl_state'
    hooks = open(os.path.join(ROOT, 'include', 'd2d_hooks.h')).read()
    assert re.findall(r'^int\s+(d2d_\w+)\s*\(', hooks, flags=re.M) == ['d2d_' + n for n in A.HIP_ONLY_ENTRY_POINTS]
    assert 'pow2_array' in A.HIP_ONLY_ENTRY_POINTS and 'pow2_array' in A.OPTIONAL and 'pow2_array' not in A.ENTRY_POINTS
    lib, fn = _lib.load_library()
    assert fn['pow2_array'](None, None, 5, None) == -1 and fn['pow2_array'](None, None, 0, None) == 0
    assert _lib.HipBackend.supports_device_owl_gaze


def _plan(pkg, B, **kw):
    from drone2d_amd import host_init, device_plugins
    A = pkg._abi
    p = pkg.with_defaults(pkg.Params(planner='Primitive', gaze_method='Owl', agent_number=10, agent_radius=15,
                                     agent_max_speed=20, drone_max_speed=40, map_id=1, **kw))
    cfg = host_init.derive_cfg(p, B=B, N=10, T=1, planner_mode=A.PLANNER_EXTERNAL, kf_enabled=True)
    plan = A.Plan()
    for k, v in device_plugins.build_tables(p, cfg, need_acos=False, owl=True)[0].items():
        setattr(plan, k, v)
    return p, cfg, plan


@pytest.mark.parametrize('planner', [1, 0])
def test_launch_shape_with_owl_is_that_of_no_gaze(pkg, planner):
    """The Owl stage uses no LDS: the persistent launch keeps exactly the geometry of D2D_GAZE_NONE."""
    from drone2d_amd import _lib
    A = pkg._abi
    _, cfg, plan = _plan(pkg, 4096)
    plan.planner, plan.launch_args = planner, 1          # any non-null launch_args: the persistent path (nothing is dereferenced)
    shapes = []
    for g in (A.GAZE_NONE, A.GAZE_OWL):
        plan.gaze = g
        shapes.append(_lib.launch_shape(cfg, plan))
    assert shapes[0] == shapes[1] and shapes[1][0] == 1, shapes
    plan.planner, plan.gaze = 0, A.GAZE_OWL              # Owl alone still takes the persistent launch (as LookAhead does)
    import closed_loop_cases as CL
    assert CL.closed_loop_path(cfg, plan) == 'k_closed<1>'


def test_bad_owl_plans_are_refused_without_gpu(pkg):
    """Owl without its table, its state, the trackers or a positive yaw rate limit is refused before any launch; 4 stays an
    unknown gaze value."""
    from drone2d_amd import _lib
    A = pkg._abi
    _, fn = _lib.load_library()
    _, cfg, plan = _plan(pkg, 4)
    st = A.State()
    for name, _ in A.State._fields_:
        setattr(st, name, 1)
    for name in A.PLAN_TABLES + A.PLAN_STATE:
        setattr(plan, name, 1)
    plan.planner, plan.gaze = A.PLAN_NONE, A.GAZE_OWL

    def refused(what, entry='gaze_stage'):
        args = (C.byref(cfg), C.byref(st), C.byref(plan), None) if entry == 'gaze_stage' else \
               (C.byref(cfg), C.byref(st), C.byref(plan), 1, 0, None, None)
        return fn[entry](*args) == -1 and what in fn['last_error']().decode()
    for field in ('owl_tab', 'owl_state'):
        setattr(plan, field, None)
        assert refused('owl_tab and owl_state'), field
        assert refused('owl_tab and owl_state', 'closed_loop'), field
        setattr(plan, field, 1)
    for bad in (0.0, -80.0, math.nan):
        plan.yaw_rate_max = bad
        assert refused('yaw_rate_max'), bad
    plan.yaw_rate_max = 80.0
    st.kf = None
    assert refused('kf')
    st.kf, cfg.kf_enabled = 1, 0
    assert refused('Kalman trackers')
    cfg.kf_enabled = 1
    st.action = None
    assert refused('action')
    st.action, plan.gaze = 1, 4
    assert refused('unknown gaze')


def test_owl_is_refused_on_a_backend_without_the_stage(pkg, oracle):
    """The CPU oracle has no Owl stage: a device Owl there is an error that names the policy, not a silent GAZE_NONE."""
    from drone2d_amd import vec_env, runner
    p = pkg.Params(planner='Primitive', gaze_method='Owl', agent_number=4, agent_radius=10, map_id=1)
    with pytest.raises(NotImplementedError, match='Owl'):
        vec_env.VecDrone2DEnv(p, 2, backend=oracle, planner='Primitive', device_plugins=True, gaze='Owl')
    with pytest.raises(NotImplementedError, match='Owl'):
        runner.ExperimentBatch(p, 2, device='cpu', backend=oracle)


def test_owl_table_equals_the_reference_expressions(pkg):
    from drone2d_amd import device_plugins as DP
    A = pkg._abi
    for kw in (dict(), dict(drone_max_yaw_speed=120, drone_view_range=120, drone_view_depth=100, dt=0.2), dict(drone_max_yaw_speed=40, dt=0.05)):
        p, _, _ = _plan(pkg, 1, **kw)
        tab = DP.owl_table(p)
        assert tab.shape == (A.OWL_TAB_LEN,) and tab.dtype == np.float64
        top = p.drone_max_yaw_speed
        u_space = np.arange(-top, top, top / 10)                                        # yaw_planner.py:161
        assert len(u_space) == A.OWL_NRATE
        yaws = u_space * 0.8                                                            # :204
        for i in range(A.OWL_NRATE):
            assert tab[A.OWL_T_RATE + i] == u_space[i] and tab[A.OWL_T_RATE08 + i] == yaws[i]
            assert tab[A.OWL_T_TURN + i] == abs(math.radians(u_space[i] * 0.8))         # :215
            assert tab[A.OWL_T_ACT + i] == u_space[i] / top                             # :222
        for i, d_i in enumerate(np.arange(0, 360, 10)):                                 # :177-178
            assert (tab[A.OWL_T_DIR + 2 * i], tab[A.OWL_T_DIR + 2 * i + 1]) == (math.cos(math.radians(d_i)), math.sin(math.radians(d_i)))
        assert (tab[A.OWL_T_FOV], tab[A.OWL_T_DEPTH]) == (p.drone_view_range, p.drone_view_depth)
        assert tab[A.OWL_T_HOLD] == int(0.8 // p.dt) - 1 == OM.hold_calls(p.dt)         # :220
        assert not tab[A.OWL_T_HOLD + 1:].any()
        m = OM.OwlModel.from_params(p)
        assert m.rates == [float(v) for v in tab[:A.OWL_NRATE]] and m.hold == tab[A.OWL_T_HOLD]
    assert OM.hold_calls(0.1) == 7                     # 0.8 // 0.1 is 7.0 in floats: 8 calls per decision
    p, cfg, _ = _plan(pkg, 1)
    assert 'owl_tab' not in DP.build_tables(p, cfg, need_acos=False)[1]                 # built only when asked for
    p.dt = 1.0
    with pytest.raises(NotImplementedError, match='dt'):                                # int(0.8 // 1.0) - 1 < 0
        DP.build_tables(p, cfg, need_acos=False, owl=True)


def _run_episode(pkg, oracle, fixture, case):
    """The episode on the env facade (oracle backend) under gaze.Owl, with the scalar model fed the same observations: per
    decision the policy's 20 costs (np.argmin's argument), its scores and its action against the model's."""
    from drone2d_amd import env as envmod, gaze
    fx = load(fixture)
    kw = json.loads(str(fx[f'r{case}_cfg']))
    p = pkg.Params(debug=True, **kw)
    p.render = False
    env = envmod.Drone2DEnv2(p, device='cpu', backend=oracle)
    pol, model = gaze.policy_list['Owl'](p), OM.OwlModel.from_params(env.params)
    real, seen = np.argmin, []

    def spy(a, *k, **kws):
        if np.shape(a) == (OM.NRATE,):
            seen.append(np.array(a, dtype=np.float64))
        return real(a, *k, **kws)
    out = dict(acts=[], scores=[], decisions=0, nan=0, active=0, multi=0, not_prefix=0, fx=fx, case=case)
    np.argmin = spy
    try:
        done = False
        while not done:
            info = env.info
            d = info['drone']
            trk = [(t.active is True, [float(v) for v in t.mu_upds[-1][:, 0]]) for t in d.trackers]
            args = (float(d.x), float(d.y), float(d.yaw), float(d.velocity[0]), float(d.velocity[1]),
                    float(info['target'][0]), float(info['target'][1]), trk)
            seen.clear()
            a = pol.plan(info)
            want = model.plan(*args)
            tag = f'{fixture} r{case} step {len(out["acts"]) + 1}'
            assert model.decided == bool(seen), tag
            if model.decided:
                ref, mine = seen[-1], np.array(model.costs)
                assert np.array_equal(ref.view(np.int64), mine.view(np.int64)) or (np.isnan(ref).all() and np.isnan(mine).all()), tag
                act = [i for i, (on, _) in enumerate(trk) if on]
                out['decisions'] += 1
                out['nan'] += bool(np.isnan(ref).all())
                out['active'] += bool(act)
                out['multi'] += len(act) >= 2
                out['not_prefix'] += bool(act) and act != list(range(len(act)))
            assert np.array_equal(np.array(model.score), pol.score), tag
            assert float(a) == want, tag
            assert (len(pol.queue), float(pol.queue[-1]) if pol.queue else model.rate) == (model.left, model.rate), tag
            out['acts'].append(float(a))
            out['scores'].append(np.array(pol.score))
            _, _, done, _ = env.step(a)
    finally:
        np.argmin = real
    return out


@pytest.fixture(scope='module')
def episodes(pkg, oracle):
    return [_run_episode(pkg, oracle, f, c) for f, c in EPISODES]


def test_model_equals_the_host_policy_on_every_golden_decision(episodes):
    """(the comparisons are the assertions of _run_episode)  The facade's episodes are the reference's: every action equals the
    fixture's, and for the new fixture so do the scores after every plan() call."""
    for ep in episodes:
        fx, i = ep['fx'], ep['case']
        acts, want = np.array(ep['acts']), fx[f'r{i}_actions']
        assert len(acts) == len(want) and np.array_equal(acts.view(np.int64), want.view(np.int64)), i
        if f'r{i}_scores' in fx.files:
            assert np.array_equal(np.array(ep['scores']), fx[f'r{i}_scores']), i


def test_the_golden_episodes_are_not_a_vacuous_net(episodes):
    """What the episodes must exercise for the comparisons to mean something; the two episodes of host_gaze_rows alone meet every
    bound."""
    old = episodes[:2]
    assert sum(ep['nan'] for ep in old) >= 3                       # the drone at rest: every cost NaN, candidate 0
    assert sum(ep['active'] for ep in old) >= 30                   # decisions with an active tracker
    assert len(set(old[0]['acts'])) >= 9                           # distinct actions in case 3
    assert sum(ep['not_prefix'] for ep in old) >= 30               # the active set is not a prefix: the zip quirk decides
    assert sum(ep['multi'] for ep in old) >= 10                    # two or more active trackers
    for ep in episodes[2:]:
        assert ep['decisions'] >= 10 and ep['nan'] >= 1
