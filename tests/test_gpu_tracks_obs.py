"""tracks_obs=True on the device (include/d2d_tracks.h: d2d_tracks_update of libd2d_tracks.so): the reference's recorded episodes
through the library step for step, the handmade cases through the launch alone over poisoned buffers, a random soak of tracker states
against the numpy model of tests/tracks_model.py, the skip rule, and an action stream and a batch of episodes with the channel
against the same without it.  Every comparison is exact equality of integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import action_stream_cases as AC
import tracks_cases as TC
import tracks_model as TM
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu


def _env(hip, p, B, **kw):
    from drone2d_amd import vec_env
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', p.planner)
    return vec_env.VecDrone2DEnv(p, B, backend=hip, **kw)


def _step(env, action):
    env._set_action(action)
    env._jerk_step(True) if env.jerk is not None else env._plugins_step()


def _launch(hip):
    return lambda cfg, st, tr: hip.tracks_update(cfg, st, tr)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('i', range(TC.EPISODES))
def test_the_recorded_episodes_through_the_library(pkg, hip, i):
    """Primitive under CVM and RVO, Jerk_Primitive with var_cam = 2 (the device draws the noise), a start next to the map's corner:
    the window after every step for the default margin, and for margin 0 every tenth step"""
    assert hip.supports_tracks_obs
    ep = TC.episode(i)
    p = TC.params_of(pkg, ep)
    kw = dict(jerk_tie=TC.tie_table()) if p.planner == 'Jerk_Primitive' else {}
    env, env0 = _env(hip, p, 1, tracks_obs=True, **kw), _env(hip, p, 1, tracks_obs=True, tracks_margin=0, **kw)
    assert TC.replay(env, ep, _step, margin0=env0) == len(ep['action'])
    keep = [t.clone() for t in (env.track_win, env.tracks['obs'], env.track_cells, env.tracks['last_step'])]
    _step(env, torch.zeros(1, dtype=torch.float64, device=env.device))
    env.sync()
    assert all(torch.equal(a, b) for a, b in zip(keep, (env.track_win, env.tracks['obs'], env.track_cells, env.tracks['last_step'])))


# ---------------------------------------------------------------------------------------------------------------- 2. handmade
@pytest.mark.parametrize('k', range(5))
def test_handmade_cases_through_the_launch_alone(pkg, hip, k):
    """every set is one launch of five envs, one more than a block's four waves: tests/tracks_cases.handmade_sets"""
    hs = TC.handmade_sets(pkg)[k]
    cfg = TC.cfg_of(hs['params'], 5, hs['N'])
    assert (cfg.W, cfg.H, cfg.L) == [(50, 50, 33), (50, 50, 33), (25, 19, 5), (25, 19, 33), (50, 50, 33)][k]
    alone, cells = TC.run_handmade(hs, _launch(hip), device=hip.device, sync=hip.sync)
    assert alone == TC.expected_handmade(hs['name']) and (0 < cells < 5 * cfg.L * cfg.L if hs['N'] else cells == 0)


def test_a_skipped_env_keeps_its_poison(pkg, hip):
    hs = TC.handmade_sets(pkg)[0]
    skipped = [e for e, q in enumerate(hs['envs']) if q['steps'] == q['last']]
    assert skipped == [4]
    cfg, st, tr, t = TC.pack(hs, hip.device)
    hip.tracks_update(cfg, st, tr)
    hip.sync()
    win, cells, last = (t[k].cpu().numpy() for k in ('win', 'cells', 'last_step'))
    assert (win[4] == TC.POISON).all() and cells[4] == TC.POISON32 and last[4] == 4
    assert not (win[:4] == TC.POISON).all(axis=(1, 2)).any() and (cells[:4] >= 0).all() and last[:4].tolist() == [3, 7, 1, 9]


# ---------------------------------------------------------------------------------------------------------------- 3. random soak
def test_random_soak_against_the_model(pkg, hip):
    """192 envs of seeded tracker states on the default map in one launch: N = 9, 0 .. 9 of them active, means inside the map and up
    to 150 px outside it, speeds up to 60 px / s, radii 3 .. 17, the drone anywhere on the map.  Coverage, not tolerance: windows of
    every kind have to occur, or the test has not looked where the launch can go wrong"""
    B, N = 192, 9
    rs = np.random.RandomState(29)
    envs = []
    for e in range(B):
        n_on = e % (N + 1)
        on = np.zeros(N, dtype=int)
        on[rs.permutation(N)[:n_on]] = 1
        trk = [(int(on[q]), rs.uniform(-150, 650), rs.uniform(-150, 650), rs.uniform(-60, 60), rs.uniform(-60, 60), rs.uniform(3, 17)) for q in range(N)]
        envs.append(TC._env(rs.uniform(0, 499.9), rs.uniform(0, 499.9), trk, steps=e + 1, last=e))
    hs = dict(name='soak', params=pkg.Params(planner='Primitive', agent_number=N), N=N, samples=TC.SAMPLES, margin=5.0, envs=envs)
    cfg, st, tr, t = TC.pack(hs, hip.device)
    hip.tracks_update(cfg, st, tr)
    hip.sync()
    win, cells, last = (t[k].cpu().numpy() for k in ('win', 'cells', 'last_step'))
    empty = full_k = 0
    for e, q in enumerate(envs):
        trk = np.array(q['trackers'])
        want = TM.window((q['x'], q['y']), trk[:, 1:5], trk[:, 0], trk[:, 5], cfg, 5.0, TC.SAMPLES)
        assert np.array_equal(win[e], want), (e, np.argwhere(win[e] != want)[:5].tolist())
        assert cells[e] == (want != 0).sum() and last[e] == e + 1, e
        empty += int(not want.any())
        full_k += int(want.max() == TC.SAMPLES)
    assert empty >= B // (N + 1) and full_k > 20 and int((win != 0).sum()) > 20 * B, (empty, full_k)


# ---------------------------------------------------------------------------------------------------------------- 4. with and without
def test_a_stream_with_the_channel_equals_the_stream_without(pkg, hip):
    """8 slots, 16 episodes, a turn every 4 steps: equal rows, the model's window after every step, zeros in a refilled slot"""
    slots, M = 8, 16
    p = AC.params_of(pkg, 'Primitive-CVM', drone_view_range=120)
    refills, frozen, nonzero = TC.stream_pair(lambda q, n, on: _env(hip, q, n, tracks_obs=on, worlds='device'), p, slots, M)
    assert refills == M - slots and frozen > 0 and nonzero > 0


def test_run_episodes_of_64_envs_with_and_without_the_channel(pkg, hip):
    from drone2d_amd import runner
    p = pkg.Params(planner='Primitive', gaze_method='LookAhead', agent_number=10, agent_radius=10, agent_max_speed=40, drone_max_speed=40,
                   drone_view_range=120, max_flight_time=4, map_id=300)
    a, b = (_env(hip, p, 64, gaze='LookAhead', worlds='device', tracks_obs=on) for on in (True, False))
    assert a.run_episodes() == b.run_episodes()
    a.sync(), b.sync()
    assert np.array_equal(runner.batch_records(a), runner.batch_records(b)) and bool(a.state.flags[:, A.F_DONE].all())
    for k, v in a.state.t.items():
        assert torch.equal(v.reshape(-1).view(torch.uint8), b.state.t[k].reshape(-1).view(torch.uint8)), k
    assert torch.equal(a.tracks['last_step'], a.state.counters[:, A.C_STEPS])
    nonzero = 0
    for e in range(0, 64, 4):                                       # the terminal windows, the model's of the terminal state
        pose, mu, active, radius = TC.env_tracks(a, e)
        want = TM.window(pose, mu, active, radius, a.cfg, 5.0, TC.SAMPLES)
        TC.check_window(a, want, e=e)
        nonzero += int(want.any())
    assert nonzero > 0


# ---------------------------------------------------------------------------------------------------------------- 5. the library
def test_the_version_symbol_and_the_refusals(pkg, hip):
    import copy
    from drone2d_amd import _lib
    lib, fn = _lib.load_tracks_library()
    assert fn['version']() == A.D2D_TRACKS_VERSION == 1
    env = _env(hip, AC.params_of(pkg, 'Primitive-CVM'), 1, tracks_obs=True)
    hip.tracks_update(env.cfg, env._st, env._tracks)
    big = copy.copy(env.cfg)
    big.L = 129
    assert hip.tfn['update'](C.byref(big), C.byref(env._st), C.byref(env._tracks), None) == -4
    assert b'64 KiB of LDS' in hip.tfn['last_error']()
    assert hip.tfn['update'](C.byref(env.cfg), C.byref(env._st), None, None) == -1
