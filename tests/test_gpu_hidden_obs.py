"""Hidden steps of the persistent closed loop (run with -m gpu).  Inside k_closed an env's observation (obs_local, obs_yaw) is written
only on the last step of a launch and on the step whose collision stage ended the env's episode (include/d2d.h, d2d_closed_loop;
csrc/d2d_hip.hip, hidden_stages): every other step runs the act phase without the observation stage.  After a launch every env must
hold exactly the bytes it held when every step wrote the observation.

For every case two envs on the same worlds, one of them with D2D_OBS_EVERY_STEP=1 in the environment (read at every call: every
step takes the visible variant): calls of 1, 2 and 3 steps and one longer call under CONTINUE, RESET and FREEZE, every array of the
env state, the plugin tables and _result() compared bit for bit after every call, and both against the oracle, which is stepped one
step at a time and so tells on which step of the longer call an episode ended."""
import contextlib
import os

import numpy as np
import pytest
import torch

import closed_loop_cases as CL
from test_gpu_closed_loop_paths import SCRATCH, ref_step
from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import _worlds
from test_plan_spec_cpu import matches, spec  # noqa: F401  (`spec`: the host build of d2d_plan_spec.h, a fixture)

pytestmark = pytest.mark.gpu

SWITCH = 'D2D_OBS_EVERY_STEP'
MODES = {'continue': {}, 'reset': dict(auto_reset=True), 'freeze': dict(freeze_done=True)}
SHORT = (1, 2, 3)

# The README's world (bench.py's config 2: 10 agents of radius 15, the default plan) with the target 140 px from the start: at
# 40 px/s an episode lasts some 40 to 60 steps, so the longer call sees most of them end -- by goal or by collision -- on a step that
# is not its last.  Neither the start nor the target is a scalar of the plan: the plan stays the one the dispatch folds.
_README = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, init_pos=[60, 60], target_list=[[70, 200]])
_FAST = dict(agent_radius=15, agent_max_speed=60)
# `long`: the steps of the longer call, picked with the oracle on the CPU;
# `min_mid`: envs whose episode has to end on a step of the longer call that is not its last
CASES = [
    dict(id='readme-folded', B=64, long=60, min_mid=8, path='k_closed<1>', folded=True, gaze='Oxford', kw=dict(map_id=1, **_README)),
    dict(id='readme-safe_dist', B=64, long=60, min_mid=8, path='k_closed<1>', folded=False, safe_dist=1.0, gaze='Oxford',
         kw=dict(map_id=1, **_README)),
    dict(id='obstacle_map', B=32, long=50, min_mid=8, path='k_closed<2>', gaze='Oxford',
         kw=dict(agent_number=10, map_id=700, static_map='maps/obstacle_map.npy', **CL._NEAR, **_FAST)),
    dict(id='default-50', B=16, long=40, min_mid=4, path='k_closed<3>', gaze='Oxford',
         kw=dict(agent_number=50, agent_radius=8, agent_max_speed=60, map_id=710, **CL._NEAR)),
    dict(id='map30x40', B=16, long=40, min_mid=4, path='k_closed<0>', gaze='Oxford',
         kw=dict(agent_number=6, map_id=720, map_size=[300, 400], init_pos=[60, 60], target_list=[[200, 300]], max_flight_time=3,
                 **_FAST)),
    dict(id='map30x40-tiled', B=16, long=40, min_mid=4, path='k_closed<4>', layout='tiled', gaze='Oxford',
         kw=dict(agent_number=6, map_id=720, map_size=[300, 400], init_pos=[60, 60], target_list=[[200, 300]], max_flight_time=3,
                 **_FAST)),
    # a planner stage that is not on the device under a gaze that is: the loop's non-split site (ph_gaze_stages<D2D_ST_ALL>).  The
    # package reaches it with the NoMove plugins (no planner stage, no waypoint) and planner_mode left at D2D_PLANNER_EXTERNAL
    # plus the external planner's result in the state (adjust): a waypoint that holds every step, a few px from the start with a
    # velocity that points away from where the drone looks -- the drone stays there and turns through 170 degrees under LookAhead, so
    # its crop and obs_yaw change step after step, and 16 fast agents of radius 15 end most episodes by collision inside the call
    dict(id='lookahead-nomove', B=32, long=60, min_mid=8, path='k_closed<1>', all_site=True, gaze='LookAhead',
         kw=dict(agent_number=16, map_id=730, init_pos=[250, 250], **_FAST)),
]


@contextlib.contextmanager
def every_step(on):
    """D2D_OBS_EVERY_STEP=1 around a call (the library reads it at every d2d_closed_loop)"""
    old = os.environ.get(SWITCH)
    if on:
        os.environ[SWITCH] = '1'
    else:
        os.environ.pop(SWITCH, None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


def row_of(case, mode):
    """The case as a row of closed_loop_cases.py (what test_gpu_closed_loop_paths.ref_step reads)"""
    return dict(gaze=case['gaze'], policy=case['gaze'], on_done=mode, path=case['path'], null_box=False)


def planner_of(case):
    return 'NoMove' if case.get('all_site') else 'Primitive'


def adjust(case, env):
    from drone2d_amd import _abi as A
    if 'safe_dist' in case:                 # one parameter away from the default plan: k_closed<1, false>
        env._plan.safe_dist += case['safe_dist']
    if case.get('all_site'):
        env.cfg.planner_mode = A.PLANNER_EXTERNAL
        # the external planner's result, as the control stage reads it from the state: a waypoint that holds every step
        for st in (env.state, env.init_state):
            e = torch.arange(env.num_envs, dtype=torch.float64)
            wp = torch.stack([246.0 + 3.0 * (e % 4), 246.0 + 3.0 * ((e // 4) % 4), -6.0 - 2.0 * (e % 3), -30.0 + (e % 16), 0.0 * e, 0.0 * e], dim=1)
            st.wp.copy_(wp.to(st.wp.device))
            st.plan_ok.fill_(1)
            st.wp_valid.fill_(1)


def ref_env(pkg, oracle, case):
    from drone2d_amd import vec_env
    p = pkg.Params(planner=planner_of(case), gaze_method=case['gaze'], **case['kw'])
    ref = vec_env.VecDrone2DEnv(p, case['B'], backend=oracle, planner=planner_of(case), device_plugins=True,
                                gaze='external' if case['gaze'] == 'LookAhead' else case['gaze'])
    adjust(case, ref)
    return p, ref


def ref_call(pkg, ref, case, mode, policy, n):
    """The oracle through one call of `n` steps, one step at a time: which envs ended an episode on a step that was not the call's
    last, the observation after the call's first step and the one before it"""
    A = pkg._abi
    row, seen = row_of(case, mode), dict(done=False, active=0, traj=False)
    before = ref.state.obs_local.clone()
    mid = np.zeros(ref.num_envs, bool)
    first = None
    for t in range(n):
        # (a frozen env is not stepped again: its flag is not an episode ending on this step)
        live = ref.state.flags[:, A.F_DONE].numpy() == 0 if mode == 'freeze' else np.ones(ref.num_envs, bool)
        ref_step(pkg, ref, row, policy, seen)
        if t == 0:
            first = ref.state.obs_local.clone()
        if t < n - 1:
            mid |= live & (ref.state.flags[:, A.F_DONE].numpy() != 0)
    return dict(mid=mid, first=first, before=before)


def _snapshot(env):
    env.sync()
    out = {'s.' + k: v.cpu() for k, v in env.state.t.items()}
    out.update({'p.' + k: v.cpu() for k, v in env.plugins.t.items() if k not in SCRATCH})
    obs, reward, done, info = env._result()
    out.update({'r.obs.' + k: v.cpu() for k, v in obs.items()})
    out.update({'r.info.' + k: v.cpu() for k, v in info.items()})
    out.update({'r.reward': reward.cpu(), 'r.done': done.cpu()})
    return out


def _same(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.dtype == y.dtype and x.shape == y.shape, f'{tag}: {k}'
        if not np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)):      # bit for bit, floats included
            raise AssertionError(f'{tag}: {k} differs at {(x != y).nonzero()[:5].tolist()}')


def _devices(pkg, hip, case, p, worlds):
    from drone2d_amd import vec_env
    envs = []
    for _ in range(2):
        env = vec_env.VecDrone2DEnv(p, case['B'], backend=hip, planner=planner_of(case), device_plugins=True, gaze=case['gaze'],
                                    worlds=worlds, grid_layout=case.get('layout', 'rowmajor'))
        adjust(case, env)
        envs.append(env)
    return envs


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['id'])
def test_hidden_steps_leave_what_every_step_left(pkg, hip, oracle, spec, case, mode):
    p, ref = ref_env(pkg, oracle, case)
    worlds = _worlds(ref)
    hidden, every = _devices(pkg, hip, case, p, worlds)
    assert CL.closed_loop_path(hidden.cfg, hidden._plan) == case['path']
    if 'folded' in case:
        assert matches(spec, hidden.cfg, hidden._plan) == case['folded']
    if case.get('all_site'):
        assert hidden._plan.planner == pkg._abi.PLAN_NONE and hidden._plan.gaze != pkg._abi.GAZE_NONE
    from drone2d_amd import gaze as G
    policy = G.LookAhead(ref.params) if case['gaze'] == 'LookAhead' else None
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        t = 0
        for n in SHORT + (case['long'],):
            call = ref_call(pkg, ref, case, mode, policy, n)
            with every_step(True):
                every.closed_loop(n, **MODES[mode])
                every.sync()
            with every_step(False):
                hidden.closed_loop(n, **MODES[mode])
                hidden.sync()
            t += n
            tag = f"{case['id']} {mode} after step {t}"
            _same(_snapshot(hidden), _snapshot(every), tag)
            _assert_same(hidden, ref, tag)
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    # the longer call did what it is there for: episodes ended on steps the host cannot see
    n_mid = int(call['mid'].sum())
    print(f"{case['id']} {mode}: {n_mid} of {case['B']} envs ended an episode inside the {case['long']}-step call")
    assert n_mid >= case['min_mid'], (case['id'], mode, n_mid)
    if mode == 'freeze':
        # a frozen env's observation is the one of the step that ended its episode: neither what the launch found nor what its first
        # step wrote (a stale crop must not pass)
        obs = hidden.state.obs_local.cpu()
        ended = np.flatnonzero(call['mid'])
        fresh = [e for e in ended if not torch.equal(obs[e], call['first'][e]) and not torch.equal(obs[e], call['before'][e])]
        assert len(fresh) >= case.get('min_fresh', case['min_mid']), (case['id'], len(fresh), len(ended))


def test_single_step_calls_are_all_visible(pkg, hip, oracle):
    """closed_loop(1) twenty times: every step is the last of its launch, so every step is visible"""
    case = CASES[0]
    p, ref = ref_env(pkg, oracle, case)
    hidden, every = _devices(pkg, hip, case, p, _worlds(ref))
    for t in range(20):
        with every_step(True):
            every.closed_loop(1, auto_reset=True)
        with every_step(False):
            hidden.closed_loop(1, auto_reset=True)
        _same(_snapshot(hidden), _snapshot(every), f'single steps, step {t + 1}')
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        ref.closed_loop(20, auto_reset=True)
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    _assert_same(hidden, ref, 'single steps, after step 20')
