"""swept_obs=True without a GPU (include/d2d_swept.h through tests/swept_backend.py, whose two launches are the numpy model of
tests/swept_model.py): the model against the reference's recorded maps step for step, a stream with and without the channel, the
refusals, Jerk_Primitive's zeros and the unchanged default."""
import numpy as np
import pytest
import torch

import action_stream_backend as AB
import action_stream_cases as AC
import swept_backend as SB
import swept_cases as SC
from drone2d_amd import _abi as A


def test_the_fixture_covers_what_it_is_for():
    trunc, empty, longest, lost = SC.coverage()
    assert trunc >= 5 and empty >= 5 and longest > 128 and lost >= 1, (trunc, empty, longest, lost)


@pytest.mark.parametrize('i', range(SC.EPISODES))
def test_the_model_against_the_reference(pkg, i):
    ep = SC.episode(i)
    env = SB.env_of(SC.params_of(pkg, ep), 1, swept_obs=True)
    assert SC.replay(env, ep) == len(ep['action'])


def test_a_stream_with_and_without_the_channel(pkg):
    """12 short episodes through 3 slots: rows, terms and local_map are identical at every step; a refilled slot has a zero swep_map at
    its step 0; a done slot keeps its terminal crop until the turn"""
    p = AC.params_of(pkg, 'Primitive-CVM')
    slots, M = 3, 12
    a = AB.env_of(p, slots, backend=SB.SweptTurnBackend().of(p), swept_obs=True).action_stream(M, refill_every=4)
    b = AB.env_of(p, slots).action_stream(M, refill_every=4)
    assert a.env.swept is not None and b.env.swept is None
    info = a.result()[3]
    kept, refills, marked = {}, 0, 0
    for call in range(2000):
        if a.finished_now() >= M:
            break
        last = info['episode'].clone()
        turned = a.turn()
        assert b.turn() == turned
        obs, _, done, info = a.result()
        for e in range(slots):
            if int(info['episode'][e]) != int(last[e]) and int(info['episode'][e]) >= 0:     # refilled: step 0 of a fresh world
                assert turned and int(info['steps'][e]) == 0 and not bool(done[e])
                assert not obs['swep_map'][e].any() and not a.env.swept_map[e].any() and int(a.env.swept_count[e]) == 0
                kept.pop(e, None)
                refills += 1
            elif e in kept:                                                                  # done, not yet turned: the terminal crop
                assert bool(done[e]) and torch.equal(obs['swep_map'][e], kept[e])
        act = AB.policy(info['episode'], info['steps'])
        oa, ta, da, ia = a.step(act)
        ob, tb, db, ib = b.step(act)
        assert torch.equal(a.rows, b.rows) and torch.equal(da, db)
        assert all(torch.equal(ta[k], tb[k]) for k in ta) and all(torch.equal(ia[k], ib[k]) for k in ia)
        assert torch.equal(oa['local_map'], ob['local_map']) and torch.equal(oa['yaw_angle'], ob['yaw_angle'])
        assert ob['swep_map'].data_ptr() == ob['local_map'].data_ptr() and oa['swep_map'].data_ptr() != oa['local_map'].data_ptr()
        marked += int(oa['swep_map'].any())
        for e in range(slots):
            if bool(da[e]) and e not in kept and bool(ia['live'][e]):
                kept[e] = oa['swep_map'][e].clone()
        info = ia
    a.close(), b.close()
    assert torch.equal(a.rows, b.rows) and int((a.rows[:, 0] > 0).sum()) == M
    assert refills == M - slots and marked > 10


def test_reset_gives_the_masked_envs_a_zero_map(pkg):
    p = AC.params_of(pkg, 'Primitive-CVM')
    env = SB.env_of(p, 2, swept_obs=True)
    for _ in range(3):
        env._set_action(torch.zeros(2, dtype=torch.float64))
        env._plugins_step()
    assert env.swept_map[0].any() and env.swept_map[1].any() and (env.swept_count > 0).all() and env._result()[0]['swep_map'][1].any()
    keep = env.swept_map[0].clone()
    env.reset(torch.tensor([0, 1], dtype=torch.uint8))
    assert torch.equal(env.swept_map[0], keep) and not env.swept_map[1].any() and int(env.swept_count[1]) == 0
    assert not env._result()[0]['swep_map'][1].any() and env._result()[0]['swep_map'][0].any()


def test_the_refusals(pkg):
    from drone2d_amd import vec_env
    p = AC.params_of(pkg, 'Primitive-CVM')
    with pytest.raises(NotImplementedError, match=r'NoMove\.replan_check returns the explored map itself'):
        vec_env.VecDrone2DEnv(p, 1, device='cpu', backend=SB.SweptOracleBackend(), planner='NoMove', device_plugins=True, gaze='external',
                              swept_obs=True)
    with pytest.raises(RuntimeError, match='swept_obs=True needs device_plugins=True'):
        vec_env.VecDrone2DEnv(p, 1, device='cpu', backend=SB.SweptOracleBackend(), planner='Primitive', swept_obs=True)
    from stepped_backend import SteppedOracleBackend
    with pytest.raises(NotImplementedError, match=r'oracle\+rvo_host\+live has no swept-map launches \(include/d2d_swept\.h'):
        SB.env_of(p, 1, backend=SteppedOracleBackend(), swept_obs=True)
    env = SB.env_of(p, 1, swept_obs=True)
    with pytest.raises(NotImplementedError, match=r'closed_loop\(\): swept_obs=True.*action_stream\(\) / policy_step\(\) / run_episodes\(\)'):
        env.closed_loop(1)
    wide = AC.params_of(pkg, 'Primitive-CVM', map_size=[2570, 500], agent_number=2)
    with pytest.raises(NotImplementedError, match=r'a map of 257 x 50 cells.*at most 256 x 256'):
        SB.env_of(wide, 1, swept_obs=True)
    assert SB.env_of(wide, 1).swept is None                    # without the channel the same map is taken
    with pytest.raises(RuntimeError, match='swept_obs=True'):
        SB.env_of(p, 1).swept_map


def test_the_per_stage_path_is_the_one_a_stream_takes(pkg):
    """with the channel a Primitive env under CVM steps stage by stage; without it, through closed_loop as before"""
    p = AC.params_of(pkg, 'Primitive-CVM')
    calls = []
    for swept in (False, True):
        env = SB.env_of(p, 1, swept_obs=swept)
        log = []
        for name in ('closed_loop', 'swept_mark', 'plan_stage_live', 'swept_crop', 'run_stages'):
            fn = getattr(env.backend, name)
            setattr(env.backend, name, lambda *a, _n=name, _f=fn: (log.append(_n), _f(*a))[1])
        env._episode_steps(1)
        calls.append(log)
    assert calls[0] == ['closed_loop']
    assert calls[1] == ['run_stages', 'swept_mark', 'plan_stage_live', 'run_stages', 'swept_crop']


def test_jerk_primitive_gives_zeros(pkg):
    p = AC.params_of(pkg, 'Jerk-CVM')
    a = SB.env_of(p, 2, backend=SB.SweptJerkBackend(), swept_obs=True)
    b = SB.env_of(p, 2, backend=SB.SweptJerkBackend())
    act = torch.full((2,), 0.5, dtype=torch.float64)
    for _ in range(5):
        oa, ob = a.step(act)[0], b.step(act)[0]
        assert oa['swep_map'].shape == oa['local_map'].shape and oa['swep_map'].dtype == torch.uint8 and not oa['swep_map'].any()
        assert torch.equal(oa['local_map'], ob['local_map']) and ob['local_map'].any()
    assert a.swept_map is None and a.swept_count is None
    with pytest.raises(NotImplementedError, match='has no swept-map launches'):
        from jerk_live_backend import LiveJerkBackend
        SB.env_of(p, 1, backend=LiveJerkBackend(), swept_obs=True)


def test_without_the_keyword_swep_map_is_local_map(pkg):
    env = SB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1)
    obs = env._result()[0]
    assert env.swept_obs is False and env.swept is None
    assert obs['swep_map'].data_ptr() == obs['local_map'].data_ptr() == env.state.obs_local.data_ptr()
    assert sorted(obs) == ['local_map', 'swep_map', 'yaw_angle']


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_the_binder_and_the_built_library_without_a_gpu(pkg):
    """include/d2d_swept.h against its ctypes mirror; the symbols are optional additions (no version moves, the oracle's surface does
    not hold them); and the built library refuses bad arguments before any launch, so this runs without a GPU"""
    import copy
    import ctypes as C
    import os
    import re
    import types
    from drone2d_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'd2d_swept.h')).read()
    assert re.findall(r'^int\s*(d2d_\w+)\(', header, re.M) == ['d2d_' + n for n in A.SWEPT_ENTRY_POINTS] == ['d2d_swept_mark', 'd2d_swept_crop']
    body = re.search(r'typedef struct \{(.*?)\} d2d_swept;', header, re.S).group(1)
    assert tuple(re.findall(r'^\s*\w+\s*\*\s*(\w+);', body, re.M)) == A.SWEPT_FIELDS == tuple(n for n, _ in A.Swept._fields_)
    assert int(re.search(r'#define\s+D2D_SWEPT_MAX_SIDE\s+(\d+)', header).group(1)) == A.SWEPT_MAX_SIDE == 256
    assert A.D2D_ABI_VERSION == 8 and 'D2D_ABI_VERSION' not in header
    assert not set(A.SWEPT_ENTRY_POINTS) & (set(A.ENTRY_POINTS) | set(A.OPTIONAL))

    class Old:
        def __getattr__(self, name):
            raise AttributeError(name)
    assert A.bind_swept(Old()) == {}
    lib, fn = _lib.load_library()
    sw = A.bind_swept(lib)
    assert sorted(sw) == sorted(A.SWEPT_ENTRY_POINTS)
    have = _lib.HipBackend.supports_swept_obs.fget
    assert have(types.SimpleNamespace(wpfn=sw)) is True and have(types.SimpleNamespace(wpfn={'swept_mark': sw['swept_mark']})) is False
    err = lambda: fn['last_error']().decode()     # noqa: E731
    c, s, p, w = A.Cfg(), A.State(), A.Plan(), A.Swept()
    assert sw['swept_mark'](C.byref(c), C.byref(s), C.byref(p), C.byref(w), None) == -2 and 'ABI' in err()
    assert sw['swept_crop'](C.byref(c), C.byref(s), C.byref(w), None) == -2 and 'ABI' in err()
    # a real cfg / state / plan (host memory: every call below is refused, or has nothing to do, before a launch)
    params = AC.params_of(pkg, 'Primitive-CVM')
    env = SB.env_of(params, 1, swept_obs=True)
    cfg, st, plan, good = env.cfg, env._st, env._plan, env._swept
    assert sw['swept_mark'](C.byref(cfg), C.byref(st), C.byref(plan), None, None) == -1 and err() == 'swept: null buffer'
    assert sw['swept_mark'](C.byref(cfg), C.byref(st), C.byref(plan), C.byref(w), None) == -1 and err() == 'swept: null buffer'
    assert sw['swept_crop'](C.byref(cfg), C.byref(st), C.byref(w), None) == -1 and err() == 'swept: null buffer'
    assert sw['swept_mark'](C.byref(cfg), C.byref(st), None, C.byref(good), None) == -1 and err() == 'null plan'
    nomove = SB.env_of(AC.params_of(pkg, 'Primitive-CVM', planner='NoMove'), 1)
    assert sw['swept_mark'](C.byref(cfg), C.byref(st), C.byref(nomove._plan), C.byref(good), None) == -1
    assert err() == "swept: the map is the Primitive planner's (D2D_PLAN_PRIMITIVE)"
    big = copy.copy(cfg)
    big.W = 257
    assert sw['swept_mark'](C.byref(big), C.byref(st), C.byref(plan), C.byref(good), None) == -4 and err() == 'swept: maps of at most 256 x 256 cells'
    assert sw['swept_crop'](C.byref(big), C.byref(st), C.byref(good), None) == -4 and err() == 'swept: maps of at most 256 x 256 cells'
    many = copy.copy(cfg)
    many.N = 4000                                  # 5 planes of 4000 doubles: 160 000 bytes and the map
    assert sw['swept_mark'](C.byref(many), C.byref(st), C.byref(plan), C.byref(good), None) == -4
    none = copy.copy(cfg)
    none.B = 0
    assert sw['swept_mark'](C.byref(none), C.byref(st), C.byref(plan), C.byref(good), None) == 0
    assert sw['swept_crop'](C.byref(none), C.byref(st), C.byref(good), None) == 0
