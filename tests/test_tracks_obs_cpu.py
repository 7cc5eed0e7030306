"""tracks_obs=True without a GPU (include/d2d_tracks.h through tests/tracks_backend.py, whose launch is the numpy model of
tests/tracks_model.py): the reference's recorded trackers and forecast windows step for step, streams with and without the channel,
every stepping path, the refusals, the host build of csrc/tracks/d2d_tracks.h against the fixture and against the model on the
handmade cases, and the header against its ctypes mirror.  Every comparison is exact equality of integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import action_stream_backend as AB
import action_stream_cases as AC
import host_build
import tracks_backend as TB
import tracks_cases as TC
import tracks_model as TM
from drone2d_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(env, action):
    env._set_action(action)
    env._jerk_step(True) if env.jerk is not None else env._plugins_step()


def _noisy_step(rng):
    """a step of a var_cam != 0 env on the oracle, which draws no measurement noise: stage by stage as env.Drone2DEnv2._perceive
    takes it, with the draws of the numpy stream the reference seeds (utils.py:603-605: randn(2) per hit agent, in agent order), and
    the channel's update behind it as every path of the env queues it.  tests/test_gpu_tracks_obs.py replays the same episode through
    the env's own path, where the device draws"""
    def step(env, action):
        env._set_action(action)
        env.run_perceive(A.ST_FSM | A.ST_AGENTS | A.ST_RAYCAST)
        noise = np.zeros((1, env.cfg.N, 2))
        for k in np.nonzero(env.state.hit[0].numpy())[0]:
            noise[0, k] = rng.randn(2)
        env.set_noise(noise)
        env.backend.run_stages(env.cfg, env._st, A.ST_DYNGRID | A.ST_TRACKER)
        env.run_jerk_plan()
        env.backend.act(env.cfg, env._st)
        env._tracks_update()
    return step


def _noise_rng(p):
    rng = np.random.RandomState(p.map_id)              # drone_v2.py:80, advanced by the 100 draws of the env's init (:51-55)
    rng.rand(100)
    return rng


def _episode_env(pkg, ep, **kw):
    p = TC.params_of(pkg, ep)
    if p.planner == 'Jerk_Primitive':
        kw['jerk_tie'] = TC.tie_table()
    return TB.env_of(p, 1, tracks_obs=True, **kw)


def test_the_fixture_covers_what_it_is_for():
    TC.assert_coverage(TC.coverage())
    assert os.path.getsize(TC.PATH) < 200 * 1000
    cfgs = [TC.episode(i)['cfg'] for i in range(TC.EPISODES)]
    assert sorted(c['planner'] for c in cfgs) == ['Jerk_Primitive', 'Primitive', 'Primitive', 'Primitive']
    assert sum(c.get('motion_profile') == 'RVO' for c in cfgs) == 1 and sum(c.get('var_cam', 0) != 0 for c in cfgs) == 1
    assert sum(c.get('init_pos') == [30, 30] for c in cfgs) == 1
    for i in range(TC.EPISODES):
        ep = TC.episode(i)
        assert len(ep['win0']) == (len(ep['win']) + 9) // 10 and any(w.any() for w in ep['win0'])


@pytest.mark.parametrize('i', range(TC.EPISODES))
def test_the_model_against_the_recorded_windows(pkg, i):
    """the definition in numpy against the reference's own get_real_pos, estimate_pos and norm, both margins"""
    ep = TC.episode(i)
    p = TC.params_of(pkg, ep)
    cfg = TC.cfg_of(p, 1, ep['active'].shape[1])
    for t in range(len(ep['action'])):
        args = (ep['pose'][t], ep['mu'][t], ep['active'][t], ep['radius'][t], cfg)
        assert np.array_equal(TM.window(*args, TC.default_margin(p), TC.SAMPLES), ep['win'][t]), t
        if t % 10 == 0:
            assert np.array_equal(TM.window(*args, 0.0, TC.SAMPLES), ep['win0'][t // 10]), t


@pytest.mark.parametrize('i', range(TC.EPISODES))
def test_the_recorded_episodes_through_the_env(pkg, i):
    """trackers, window, observation and count after every step, the terminal step included; then a further step changes nothing"""
    ep = TC.episode(i)
    env, env0 = _episode_env(pkg, ep), _episode_env(pkg, ep, tracks_margin=0)
    step = _step
    if env.params.var_cam != 0:
        assert env.jerk is not None
        own = {id(e_): _noisy_step(_noise_rng(env.params)) for e_ in (env, env0)}
        step = lambda e_, a: own[id(e_)](e_, a)      # noqa: E731
    assert TC.replay(env, ep, step, margin0=env0) == len(ep['action'])
    keep = [t.clone() for t in (env.track_win, env.tracks['obs'], env.track_cells, env.tracks['last_step'])]
    before = env.backend.tracks_updates
    _step(env, torch.zeros(1, dtype=torch.float64))
    assert env.backend.tracks_updates == before + 1
    assert all(torch.equal(a, b) for a, b in zip(keep, (env.track_win, env.tracks['obs'], env.track_cells, env.tracks['last_step'])))


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_a_stream_with_and_without_the_channel(pkg, cell):
    p = AC.params_of(pkg, cell, drone_view_range=120)
    make = lambda q, n, on: AB.env_of(q, n, backend=TB.stream_backend_for(q), tracks_obs=True) if on else AB.env_of(q, n)      # noqa: E731
    refills, frozen, nonzero = TC.stream_pair(make, p, 3, 9)
    assert refills == 9 - 3 and frozen > 0 and nonzero > 0


def test_stream_episodes_refills_show_zeros(pkg):
    """stream_episodes() (a policy of the device's) rebuilds a slot through _refill_rest: a refilled slot shows a zero window"""
    p = AC.params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    env = AB.env_of(p, 2, backend=TB.stream_backend_for(p), tracks_obs=True, gaze='Rotating')
    rounds = 0
    for finished, refill in env.stream_rounds(5, refill_every=8):
        for e in np.nonzero(refill.numpy())[0]:
            assert not bool(env.track_win[e].any()) and int(env.track_cells[e]) == 0 and int(env.tracks['last_step'][e]) == 0
            rounds += 1
    assert rounds >= 3 and int((env.stream_rows[:, 0] > 0).sum()) == 5


def test_every_stepping_path_queues_one_update_per_step(pkg):
    p = AC.params_of(pkg, 'Primitive-CVM')

    def count(env, fn):
        before = env.backend.tracks_updates
        fn()
        return env.backend.tracks_updates - before
    act = torch.zeros(2, dtype=torch.float64)
    env = TB.env_of(p, 2, tracks_obs=True)
    assert env.backend.tracks_updates == 1 and env.tracks['last_step'].tolist() == [0, 0]      # the update at construction
    assert count(env, lambda: env.step(act)) == 1
    assert count(env, env.perceive) == 0 and count(env, lambda: env.act(act)) == 1
    assert count(env, env._plugins_step) == 1
    assert env.tracks['last_step'].tolist() == [3, 3]
    assert count(env, lambda: env.reset(torch.tensor([1, 0], dtype=torch.uint8))) == 1
    assert env.tracks['last_step'].tolist() == [0, 3] and not bool(env.track_win[0].any())
    log = []
    for name in ('closed_loop', 'tracks_update'):
        fn = getattr(env.backend, name)
        setattr(env.backend, name, lambda *a, _n=name, _f=fn, **k: (log.append((_n, a[3] if _n == 'closed_loop' else None)), _f(*a, **k))[1])
    env._episode_steps(3)                                               # Primitive under CVM: its one-step persistent launch, three times
    assert log == [('closed_loop', 1), ('tracks_update', None)] * 3
    ox = TB.env_of(AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'), 2, tracks_obs=True, gaze='Oxford')
    assert count(ox, ox.policy_step) == 1 and count(ox, lambda: ox.run_episodes(max_steps=3)) == 3
    rvo = TB.env_of(AC.params_of(pkg, 'Primitive-RVO'), 2, tracks_obs=True)
    assert count(rvo, lambda: rvo._episode_steps(2)) == 2
    jp = AC.params_of(pkg, 'Jerk-CVM')
    jerk = TB.env_of(jp, 2, tracks_obs=True)
    assert count(jerk, lambda: jerk.step(act)) == 1 and count(jerk, lambda: jerk._jerk_step(True)) == 1
    assert count(jerk, lambda: jerk._episode_steps(2)) == 2
    jr = TB.env_of(AC.params_of(pkg, 'Jerk-RVO'), 2, tracks_obs=True)
    assert count(jr, lambda: jr._episode_steps(2)) == 2
    assert count(jerk, jerk.tracks_refresh) == 1 and jerk._tracks.force == 0
    # the update is the model's for the state the env is in, whatever path moved it
    for e_ in (env, ox, rvo, jerk, jr):
        for e in range(2):
            pose, mu, active, radius = TC.env_tracks(e_, e)
            TC.check_window(e_, TM.window(pose, mu, active, radius, e_.cfg, 5.0, 31), e=e)
            assert int(e_.tracks['last_step'][e]) == int(e_.state.counters[e, A.C_STEPS])


def test_tracks_refresh_sees_what_the_caller_wrote(pkg):
    env = TB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1, tracks_obs=True, tracks_samples=5, tracks_margin=0)
    env.state.active[0, 0] = 1
    env.state.kf[0, 0, :4] = torch.tensor([env.state.drone[0, 0] + 20.0, env.state.drone[0, 1], 10.0, 0.0], dtype=torch.float64)
    env._tracks_update()
    assert not bool(env.track_win.any())                                # the counter has not moved: skipped
    env.tracks_refresh()
    pose, mu, active, radius = TC.env_tracks(env)
    want = TM.window(pose, mu, active, radius, env.cfg, 0.0, 5)
    assert want.any() and int(want.max()) <= 5
    TC.check_window(env, want)


def test_without_the_keyword_nothing_is_added(pkg):
    env = TB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1)
    assert env.tracks_obs is False and env.tracks is None and env.backend.tracks_updates == 0
    env.step(torch.zeros(1, dtype=torch.float64))
    assert sorted(env._result()[0]) == ['local_map', 'swep_map', 'yaw_angle'] and env.backend.tracks_updates == 0
    for name in ('track_win', 'track_cells'):
        with pytest.raises(RuntimeError, match='tracks_obs=True'):
            getattr(env, name)
    with pytest.raises(RuntimeError, match='tracks_obs=True'):
        env.tracks_refresh()


def test_the_refusals(pkg):
    from stepped_backend import SteppedOracleBackend
    p = AC.params_of(pkg, 'Primitive-CVM')
    with pytest.raises(NotImplementedError, match=r'oracle\+rvo_host\+live has no tracker-forecast launch \(include/d2d_tracks\.h'):
        TB.env_of(p, 1, backend=SteppedOracleBackend(), tracks_obs=True)
    env = TB.env_of(p, 1, tracks_obs=True)
    with pytest.raises(NotImplementedError, match=r'closed_loop\(\): tracks_obs=True.*action_stream\(\) / policy_step\(\) / run_episodes\(\)'):
        env.closed_loop(1)
    with pytest.raises(NotImplementedError, match=r'rollout\(\): tracks_obs=True'):
        env.rollout(torch.zeros((2, 1), dtype=torch.float64))
    with pytest.raises(NotImplementedError, match=r"planner 'NoMove' with device plugins keeps no tracker radii \(trk_radius"):
        TB.env_of(AC.params_of(pkg, 'Primitive-CVM', planner='NoMove'), 1, tracks_obs=True)
    with pytest.raises(NotImplementedError, match=r"planner 'NoMove' without device plugins keeps no tracker radii \(trk_radius"):
        TB.env_of(AC.params_of(pkg, 'Primitive-CVM', planner='NoMove'), 1, tracks_obs=True, device_plugins=False, gaze=None)
    with pytest.raises(NotImplementedError, match=r"planner 'Primitive' without device plugins keeps no tracker radii \(trk_radius"):
        TB.env_of(p, 1, tracks_obs=True, device_plugins=False, gaze=None)
    with pytest.raises(ValueError, match=r'tracks_obs=True reads the Kalman trackers \(kf_enabled=True\)'):
        TB.env_of(p, 1, tracks_obs=True, kf_enabled=False)
    for bad in (0, 256, -3):
        with pytest.raises(ValueError, match=rf'tracks_samples={bad} \(1 \.\. 255'):
            TB.env_of(p, 1, tracks_obs=True, tracks_samples=bad)
    for ok in (1, 255):
        assert TB.env_of(p, 1, tracks_obs=True, tracks_samples=ok)._tracks.samples == ok
    assert TB.env_of(AC.params_of(pkg, 'Primitive-CVM', var_cam=2), 1, tracks_obs=True)._tracks.margin == 7.0
    assert TB.env_of(p, 1, tracks_obs=True, tracks_margin=0)._tracks.margin == 0.0


def test_all_four_channels_together(pkg):
    """the keys and shapes, and the other three channels bit-equal to the same env without tracks_obs"""
    p = AC.params_of(pkg, 'Primitive-CVM', drone_view_range=120)

    def build(tracks):
        b = TB.AllOracleBackend()
        b.seen_view_range = 120
        return TB.env_of(p, 2, backend=b, swept_obs=True, seen_obs=True, scan_obs=True, tracks_obs=tracks)
    a, b = build(True), build(False)
    L, R = a.cfg.L, a.cfg.R
    for t in range(12):
        act = torch.tensor([0.5, -0.25], dtype=torch.float64)
        for e_ in (a, b):
            _step(e_, act)
        oa, ob = a._result()[0], b._result()[0]
        assert sorted(oa) == ['age_map', 'local_map', 'scan', 'swep_map', 'track_map', 'yaw_angle'] and sorted(set(oa) - set(ob)) == ['track_map']
        assert {k: tuple(v.shape) for k, v in oa.items()} == dict(local_map=(2, 1, L, L), swep_map=(2, 1, L, L), yaw_angle=(2, 1), age_map=(2, 1, L, L),
                                                                  scan=(2, 2, R), track_map=(2, 1, L, L))
        assert all(torch.equal(oa[k].reshape(-1).view(torch.uint8), ob[k].reshape(-1).view(torch.uint8)) for k in ob), t
        for k, v in a.state.t.items():
            assert torch.equal(v.reshape(-1).view(torch.uint8), b.state.t[k].reshape(-1).view(torch.uint8)), (t, k)
    assert bool(oa['swep_map'].any()) and bool(oa['age_map'].any()) and bool(oa['scan'].any())


# ---------------------------------------------------------------------------------------------------------------- the host build
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    lib = host_build.shared('tracks_host.c', tmp_path_factory.mktemp('tracks'), 'libtracks_host.so')
    P = C.POINTER
    lib.tracks_host_update.argtypes = [P(A.Cfg), P(A.State), P(A.Tracks)]
    lib.tracks_host_check.argtypes = [P(A.Cfg), P(A.State), P(A.Tracks), C.c_char_p, C.c_int]
    lib.tracks_host_cell.argtypes = [C.c_double, C.c_double, C.c_int]
    lib.tracks_host_sq_threshold.argtypes = [C.c_double]
    lib.tracks_host_sq_threshold.restype = C.c_double
    return lib


def _host_launch(host):
    def launch(cfg, st, tr):
        assert host.tracks_host_update(C.byref(cfg), C.byref(st), C.byref(tr)) == 0
    return launch


@host_build.needs_fma('csrc/tracks/d2d_tracks.h fuses the distance test and the remainder of a quotient (-mfma)')
@pytest.mark.parametrize('k', range(5))
def test_the_host_build_against_the_model_on_the_handmade_cases(pkg, host, k):
    hs = TC.handmade_sets(pkg)[k]
    cfg = TC.cfg_of(hs['params'], 5, hs['N'])
    assert (cfg.W, cfg.H, cfg.L) == [(50, 50, 33), (50, 50, 33), (25, 19, 5), (25, 19, 33), (50, 50, 33)][k]
    alone, cells = TC.run_handmade(hs, _host_launch(host))
    assert alone == TC.expected_handmade(hs['name']) and (0 < cells < 5 * cfg.L * cfg.L if hs['N'] else cells == 0)


def test_the_handmade_geometry_is_what_it_claims(pkg):
    """the `near` set through the model alone: the cases its docstring names are there"""
    hs = TC.handmade_sets(pkg)[0]
    cfg = TC.cfg_of(hs['params'], 5, hs['N'])

    def win(e, only=None, also=None):
        q = hs['envs'][e]
        trk = np.array(q['trackers'])
        on = trk[:, 0].copy()
        if only is not None:
            on = (np.arange(len(on)) == only) * on
        if also is not None:
            on[also] = 1
        return TM.window((q['x'], q['y']), trk[:, 1:5], on, trk[:, 5], cfg, hs['margin'], hs['samples'])
    # two trackers reach the same cells at different samples, and the smaller sample stands
    a, b, both = win(0, only=0).astype(int), win(0, only=1).astype(int), win(0).astype(int)
    shared = (a != 0) & (b != 0)
    assert (shared & (a < b)).any() and (shared & (b < a)).any() and np.array_equal(both[shared], np.minimum(a, b)[shared])
    # ... and the inactive tracker on the drone would have changed the window
    assert both[16, 16] != 1 and win(0, also=2)[16, 16] == 1
    # a forecast that leaves the map is cut at its edge; one that starts outside the window enters it
    q = hs['envs'][1]
    assert q['trackers'][0][1] + 3.0 * q['trackers'][0][3] > 500 and win(1, only=0).any()
    enter = win(1, only=1)
    assert enter.any() and int(enter[enter != 0].min()) > 1
    # the drone in a corner: the rows and columns in front of the map stay zero
    corner = win(2)
    assert corner[16:, 16:].any() and not corner[:16].any() and not corner[:, :16].any()
    # exactly thr from a cell centre along x and along y: inside; an ulp further: outside (cell (i, j) is window [i - 9, j - 9])
    edge = win(3)
    assert edge[25 - 9, 25 - 9] == 1 and edge[19 - 9, 17 - 9] == 1 and edge[10 - 9, 11 - 9] == 0 and edge[10 - 9, 12 - 9] == 1


@host_build.needs_fma('csrc/tracks/d2d_tracks.h fuses the distance test and the remainder of a quotient (-mfma)')
@pytest.mark.parametrize('i', range(TC.EPISODES))
def test_the_host_build_against_the_fixture(pkg, host, i):
    """the recorded trackers of every step through the C loop alone, one env a step, both margins"""
    ep = TC.episode(i)
    p = TC.params_of(pkg, ep)
    T, N = ep['active'].shape
    for margin, wins, steps in ((TC.default_margin(p), ep['win'], range(T)), (0.0, ep['win0'], range(0, T, 10))):
        steps = list(steps)
        hs = dict(name=f'episode {i}', params=p, N=N, samples=TC.SAMPLES, margin=margin,
                  envs=[TC._env(ep['pose'][t, 0], ep['pose'][t, 1], [(int(ep['active'][t, q]), *ep['mu'][t, q], ep['radius'][t, q]) for q in range(N)],
                                steps=t + 1, last=t) for t in steps])
        cfg, st, tr, t_ = TC.pack(hs)
        _host_launch(host)(cfg, st, tr)
        assert np.array_equal(t_['win'].numpy(), wins), np.argwhere((t_['win'].numpy() != wins).any(axis=(1, 2)))[:5].tolist()
        assert np.array_equal(t_['cells'].numpy(), (wins != 0).reshape(len(steps), -1).sum(1))


def test_the_host_build_under_the_sanitizers(pkg, host, tmp_path):
    """the handmade sets through a stand-alone program built with AddressSanitizer and UBSan, on exactly sized heap arrays: every
    index the loop forms -- the tracker records, the boxes, the window plane -- stays inside its array"""
    import struct
    import subprocess
    records = []
    for hs in TC.handmade_sets(pkg):
        TC.run_handmade(hs, _host_launch(host), record=records)
    path = tmp_path / 'records.bin'
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(records)))
        for r in records:
            c, hs = r['cfg'], r['hs']
            f.write(struct.pack('<6i4d', c.B, c.N, c.W, c.H, c.L, hs['samples'], c.scale, c.dt, c.drone_radius, hs['margin']))
            for k in ('drone', 'counters', 'kf', 'active', 'trk_radius'):
                f.write(np.ascontiguousarray(r['inputs'][k]).tobytes())
            for v in ('before', 'first', 'forced'):
                for k in ('win', 'cells', 'last_step'):
                    f.write(np.ascontiguousarray(r[v][k]).tobytes())
    exe = host_build.sanitized(['tracks_host.c', 'tracks_host_main.c'], tmp_path, 'tracks_host_san')
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


def test_the_pieces_of_the_header(host):
    import math
    from drone2d_amd.device_plugins import sq_threshold
    rs = np.random.RandomState(1)
    vs = np.concatenate([rs.uniform(-30, 530, 2000), np.arange(-3, 53) * 10.0, np.nextafter(np.arange(1, 51) * 10.0, 0), [1e300, -1e300]])
    for s in (10.0, 3.0):
        for v in vs:
            assert host.tracks_host_cell(v, s, 50) == int(min(max(v // s, -2), 51)), (v, s)
    assert host.tracks_host_cell(float('nan'), 10.0, 50) == -2
    for r in np.concatenate([rs.uniform(0, 60, 500), [0.0, 25.0, 20.0, 27.0, 1e-160, 1e150]]):
        assert host.tracks_host_sq_threshold(r) == sq_threshold(float(r)), r
    assert host.tracks_host_sq_threshold(-1.0) == -1.0 and host.tracks_host_sq_threshold(math.nan) == -1.0


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_the_mirror_and_the_built_library_without_a_gpu(pkg, host):
    from drone2d_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'd2d_tracks.h')).read()
    assert re.findall(r'^(?:int|const char \*)\s*(d2d_tracks_\w+)\(', header, re.M) == ['d2d_tracks_version', 'd2d_tracks_last_error', 'd2d_tracks_update']
    body = re.search(r'typedef struct d2d_tracks \{(.*?)\} d2d_tracks;', header, re.S).group(1)
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);', body, re.M)
    assert tuple(n for _, n in fields) == tuple(n for n, _ in A.Tracks._fields_)
    ctype = {'int32_t': C.c_int32, 'double': C.c_double}
    for (t, n), (m, ct) in zip(fields, A.Tracks._fields_):
        assert ct is (C.c_void_p if n in A.TRACKS_POINTERS else ctype[t]), n
    assert set(A.TRACKS_BUFFERS) | {'trk_radius'} == set(A.TRACKS_POINTERS)
    assert int(re.search(r'#define\s+D2D_TRACKS_VERSION\s+(\d+)', header).group(1)) == A.D2D_TRACKS_VERSION == host.tracks_host_version()
    assert int(re.search(r'#define\s+D2D_TRACKS_MAX_SAMPLES\s+(\d+)', header).group(1)) == A.TRACKS_MAX_SAMPLES == 255
    assert host.tracks_host_struct_bytes() == C.sizeof(A.Tracks)
    d2d = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert 'tracks_update' not in d2d and 'd2d_tracks' not in d2d
    # the built library: its version, and every refusal comes before a launch, so this runs without a GPU
    lib, fn = _lib.load_tracks_library()
    assert fn['version']() == A.D2D_TRACKS_VERSION and sorted(fn) == ['last_error', 'update', 'version']
    err = lambda: fn['last_error']().decode()     # noqa: E731
    env = TB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1, tracks_obs=True)
    cfg, st, good = env.cfg, env._st, env._tracks
    up = lambda c, s, w: fn['update'](None if c is None else C.byref(c), None if s is None else C.byref(s), None if w is None else C.byref(w), None)   # noqa: E731
    assert up(None, st, good) == -1 and up(cfg, None, good) == -1 and up(cfg, st, None) == -1 and 'NULL' in err()
    assert up(A.Cfg(), st, good) == -2 and 'ABI' in err()
    assert up(cfg, A.State(), good) == -1 and err() == 'd2d_tracks_update: drone or counters is NULL'
    for name in A.TRACKS_BUFFERS:
        bad = A.Tracks.from_buffer_copy(good)
        setattr(bad, name, None)
        assert up(cfg, st, bad) == -1 and err() == 'd2d_tracks_update: a tracks buffer is NULL', name
    import copy
    for name in ('kf', 'active'):
        s2 = A.State.from_buffer_copy(st)
        setattr(s2, name, None)
        assert up(cfg, s2, good) == -1 and 'with N > 0' in err(), name
    bad = A.Tracks.from_buffer_copy(good)
    bad.trk_radius = None
    assert up(cfg, st, bad) == -1 and 'with N > 0' in err()
    for samples in (0, 256):
        bad = A.Tracks.from_buffer_copy(good)
        bad.samples = samples
        assert up(cfg, st, bad) == -1 and err() == 'd2d_tracks_update: samples is 1 .. 255'
    big = copy.copy(cfg)
    big.L = 129
    assert up(big, st, good) == -4 and '64 KiB of LDS' in err()
    why = C.create_string_buffer(256)
    assert host.tracks_host_check(C.byref(big), C.byref(st), C.byref(good), why, 256) == -4 and why.value.decode() == err()
    many = copy.copy(cfg)
    many.N = 2000
    assert up(many, st, good) == -4
    none = copy.copy(cfg)
    none.B = 0
    assert up(none, st, good) == 0
