"""The persistent closed loop with the plugins' default parameters folded in (k_closed<1, true>, csrc/d2d_plan_spec.h) against the
oracle (run with -m gpu): 16 worlds of the headline workload whose 150 steps hold a search capped at 99 expansions, one that dies on
an empty open set, successes and episodes that end and restart; the same worlds with the fold switched off (D2D_PLAN_FOLD=0), which
must give the same arrays; and four plans one parameter away from the default, which keep today's kernels and stay exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import _worlds
from test_plan_spec_cpu import HEADLINE, matches, spec  # noqa: F401  (`spec`: the host build of d2d_plan_spec.h, a fixture)

pytestmark = pytest.mark.gpu

# map_id of the 16 worlds (bench.py's config 2 is map_id = 1 + env), picked with the oracle on the CPU: in their first 150 steps
# worlds 5, 24, 34, 155, 175, 192 and 255 run searches capped at 99 expansions (192: ten in a row), world 11 searches that fail on
# an empty open set after one expansion, every world successful ones, and 11, 12, 16, 24, 155, 192 and 255 end an episode and restart
WORLDS = [1, 2, 3, 5, 11, 12, 16, 22, 24, 34, 111, 113, 155, 175, 192, 255]
STEPS, CHUNK = 150, 50
NEAR_MISSES = [dict(drone_max_speed=30), dict(drone_view_range=60), dict(drone_max_yaw_speed=60), dict(agent_number=17)]


def _arrays(env):
    """What closed_loop() returns -- obs, reward, done, every info array -- and the planner's plan_stat and traj_hdr, on the host"""
    env.sync()
    obs, reward, done, info = env._result()
    out = {'obs.' + k: v for k, v in obs.items()}
    out.update({'info.' + k: v for k, v in info.items()})
    out.update(reward=reward, done=done, plan_stat=env.plugins.t['plan_stat'], traj_hdr=env.plugins.t['traj_hdr'])
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, f'{tag}: {k} {x.dtype}{x.shape} vs {y.dtype}{y.shape}'
        if not np.array_equal(x.view(np.uint8), y.view(np.uint8)):          # bit for bit, floats included
            bad = np.argwhere(x != y)
            raise AssertionError(f'{tag}: {k} differs at {bad[:5].tolist()} ({len(bad)} elements)')


def _headline_envs(pkg, hip, oracle):
    from drone2d_amd import vec_env
    plist = [pkg.Params(**dict(HEADLINE, map_id=w)) for w in WORLDS]
    worlds = vec_env.build_worlds_of(plist)
    ref = dev = None
    if oracle is not None:
        ref = vec_env.VecDrone2DEnv(plist[0], len(WORLDS), backend=oracle, planner='Primitive', device_plugins=True, gaze='Oxford',
                                    worlds=worlds)
    if hip is not None:
        dev = vec_env.VecDrone2DEnv(plist[0], len(WORLDS), backend=hip, planner='Primitive', device_plugins=True, gaze='Oxford',
                                    worlds=worlds)
    return dev, ref


@pytest.fixture(scope='module')
def reference(pkg, oracle):
    """The oracle's run, once: its arrays after every chunk (it is stepped one step at a time: plan_stat describes the LAST search of
    an env only) and what the 150 steps held"""
    A = pkg._abi
    _, ref = _headline_envs(pkg, None, oracle)
    seen = dict(capped=0, empty=0, success=0, ended=0, restarted=0)
    chunks = []
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        prev = ref.plugins.t['plan_stat'].numpy().copy()
        for t in range(STEPS):
            was_done = ref.state.flags[:, A.F_DONE].numpy() != 0
            ref.closed_loop(1, auto_reset=True)
            ps = ref.plugins.t['plan_stat'].numpy()
            searched = ps[:, 0] != prev[:, 0]
            ok = ref.state.plan_ok.numpy() != 0
            seen['capped'] += int((searched & ~ok & (ps[:, 1] == 99)).sum())
            seen['empty'] += int((searched & ~ok & (ps[:, 1] < 99)).sum())
            seen['success'] += int((searched & ok & (ref.plugins.t['traj_hdr'].numpy()[:, 1] > 0)).sum())
            seen['ended'] += int((ref.state.flags[:, A.F_DONE].numpy() != 0).sum())
            seen['restarted'] += int((was_done & (ref.state.counters[:, A.C_STEPS].numpy() == 1)).sum())
            prev = ps.copy()
            if (t + 1) % CHUNK == 0:
                chunks.append(_arrays(ref))
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    return dict(chunks=chunks, seen=seen, ref=ref)


def _device_run(pkg, hip, spec):
    dev, _ = _headline_envs(pkg, hip, None)
    assert matches(spec, dev.cfg, dev._plan)                # the plan the dispatch folds
    out = []
    for _ in range(STEPS // CHUNK):
        dev.closed_loop(CHUNK, auto_reset=True)
        out.append(_arrays(dev))
    return dev, out


@pytest.fixture(scope='module')
def folded(pkg, hip, spec):
    assert os.environ.get('D2D_PLAN_FOLD') != '0', 'D2D_PLAN_FOLD=0 in the environment: the folded kernel would not run'
    return _device_run(pkg, hip, spec)


def test_the_worlds_hold_what_they_were_picked_for(reference):
    """A silent change of the worlds must not empty the comparison below: the oracle's own run has all four"""
    seen = reference['seen']
    assert seen['capped'] >= 1, seen        # a search that gives up at itr >= max_itr: 99 expansions
    assert seen['empty'] >= 1, seen         # a search that fails on an empty open set
    assert seen['success'] >= 1, seen       # a search that stores a trajectory
    assert seen['ended'] >= 1 and seen['restarted'] >= 1, seen


def test_folded_kernel_matches_oracle(reference, folded):
    dev, got = folded
    for i, (a, b) in enumerate(zip(got, reference['chunks'])):
        _same(a, b, f'after step {(i + 1) * CHUNK}')
    assert len(got) == len(reference['chunks']) == STEPS // CHUNK
    _assert_same(dev, reference['ref'], f'after step {STEPS}')      # and every field of the env and plugin state at the end


def test_fold_switched_off_gives_the_same_arrays(pkg, hip, spec, folded):
    """D2D_PLAN_FOLD=0 (read by the host dispatch at every call): k_closed<1> on the same plan"""
    old = os.environ.get('D2D_PLAN_FOLD')
    os.environ['D2D_PLAN_FOLD'] = '0'
    try:
        libc = C.CDLL(None)
        libc.getenv.restype = C.c_char_p
        assert libc.getenv(b'D2D_PLAN_FOLD') == b'0'        # the library's getenv sees what os.environ was given
        _, got = _device_run(pkg, hip, spec)
    finally:
        if old is None:
            del os.environ['D2D_PLAN_FOLD']
        else:
            os.environ['D2D_PLAN_FOLD'] = old
    for i, (a, b) in enumerate(zip(got, folded[1])):
        _same(a, b, f'after step {(i + 1) * CHUNK}')
    assert len(got) == len(folded[1])


@pytest.mark.parametrize('kw', NEAR_MISSES, ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_near_miss_keeps_todays_kernel_and_stays_exact(pkg, hip, oracle, spec, kw):
    from drone2d_amd import vec_env
    p = pkg.Params(**dict(HEADLINE, map_id=7, **kw))
    ref = vec_env.VecDrone2DEnv(p, 4, backend=oracle, planner='Primitive', device_plugins=True, gaze='Oxford')
    dev = vec_env.VecDrone2DEnv(p, 4, backend=hip, planner='Primitive', device_plugins=True, gaze='Oxford', worlds=_worlds(ref))
    assert not matches(spec, dev.cfg, dev._plan)
    for t in (20, 40):
        dev.closed_loop(20, auto_reset=True)
        ref.closed_loop(20, auto_reset=True)
        _same(_arrays(dev), _arrays(ref), f'after step {t}')
        _assert_same(dev, ref, f'after step {t}')
    assert int(ref.plugins.t['plan_stat'][:, 0].min()) >= 1
