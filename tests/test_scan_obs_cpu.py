"""scan_obs=True without a GPU (include/d2d_scan.h through tests/scan_backend.py, whose launch is the plain-Python model of
tests/scan_model.py): the reference's recorded rays step for step, streams with and without the channel, every stepping path, reset
and refill, the refusals, the host build of csrc/scan/d2d_scan.h against the model on the handmade poses, the header against its
ctypes mirror and the facade's `env.drone.rays`.  Every comparison is exact equality: integers, and the bit patterns of floats."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import action_stream_backend as AB
import action_stream_cases as AC
import host_build
import scan_backend as SB
import scan_cases as SC
import scan_model as SN
from drone2d_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fixture_covers_what_it_is_for():
    cov = SC.coverage()
    SC.assert_coverage(cov)
    assert os.path.getsize(SC.PATH) < 200 * 1000
    eps = [SC.episode(i) for i in range(SC.EPISODES)]
    assert [e['cfg']['planner'] for e in eps] == ['NoMove', 'Primitive', 'Primitive', 'NoMove']
    assert [len(e['action']) for e in eps][:2] == [40, 60] and len(eps[3]['action']) == 20
    assert eps[2]['cfg']['motion_profile'] == 'RVO' and eps[3]['cfg']['map_size'] == [1000, 800]
    assert [e['hit'].shape[2] for e in eps] == [2, 1, 1, 2]
    # the drone of episode (a) stands on the map's edge in five steps: no ray of those takes a sample
    assert int((eps[0]['pose'][:, 0] == 0).sum()) == 5 and cov['kinds'][0] == 250


@pytest.mark.parametrize('i', range(SC.EPISODES))
def test_the_recorded_episodes_through_the_env(pkg, i):
    """coords, kind, hit list and wall of every ray of every step; no rays before the first step"""
    ep = SC.episode(i)
    env = SB.env_of(SC.params_of(pkg, ep), 1, scan_obs=True, **SC.env_kw(ep))
    assert (env.cfg.R, env.cfg.N) == (ep['kind'].shape[1], ep['cfg']['agent_number'])
    assert SC.replay(env, ep) == len(ep['action'])
    if ep['cfg']['planner'] != 'NoMove':       # the episode is over: the env is finished and nothing moves
        assert bool(env.state.flags[0, A.F_DONE]) or i == 1
        keep = [t.clone() for t in env.scan.values()]
        if bool(env.state.flags[0, A.F_DONE]):
            SC.step_of(ep)(env, torch.zeros(1, dtype=torch.float64))
            assert all(torch.equal(a, b) for a, b in zip(keep[1:], list(env.scan.values())[1:]))


def test_the_model_is_the_reference_on_its_own(pkg):
    """the plain-Python model alone against the recorded rays of the teleport episode: the recorded pose, the agents the env holds
    behind each step"""
    ep = SC.episode(0)
    env = SB.env_of(SC.params_of(pkg, ep), 1, scan_obs=False, **SC.env_kw(ep))
    for t in range(8):
        env.state.drone[0, :3] = torch.from_numpy(ep['tele'][t].copy())
        env.step(torch.zeros(1, dtype=torch.float64))
        end, kind, hit, obs = SN.scan(ep['pose'][t], env.state.agents[0].numpy(), env.state.gt[0].numpy().reshape(-1), env.cfg, 2)
        assert np.array_equal(SC.bits(end), SC.bits(ep['coords'][t])) and np.array_equal(kind, ep['kind'][t]) and np.array_equal(hit, ep['hit'][t]), t


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_a_stream_with_and_without_the_channel(pkg, cell):
    p = AC.params_of(pkg, cell)
    cls = SB.ScanTurnJerkBackend if p.planner == 'Jerk_Primitive' else SB.ScanTurnBackend
    make = lambda q, n, scan: AB.env_of(q, n, backend=cls().of(q), scan_obs=True) if scan else AB.env_of(q, n)      # noqa: E731
    refills, frozen = SC.stream_pair(make, p, 3, 9)
    assert refills == 9 - 3 and frozen > 0


def test_stream_episodes_refills_through_the_masked_fills(pkg):
    """stream_episodes() (a policy of the device's) rebuilds a slot through _refill_rest: a refilled slot shows no rays"""
    p = AC.params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    env = AB.env_of(p, 2, backend=SB.ScanTurnBackend().of(p), scan_obs=True, gaze='Rotating')
    rounds = 0
    for finished, refill in env.stream_rounds(5, refill_every=8):
        for e in np.nonzero(refill.numpy())[0]:
            SC.check_cleared(env, int(e))
            rounds += 1
    assert rounds >= 3 and int((env.stream_rows[:, 0] > 0).sum()) == 5


def test_every_stepping_path_queues_one_snapshot_and_one_update_per_step(pkg):
    p = AC.params_of(pkg, 'Primitive-CVM')

    def count(env, fn):
        """(snapshots, updates) queued by fn()"""
        snaps, before = [], env.backend.scan_updates
        orig = env._scan_snapshot
        env._scan_snapshot = lambda: (snaps.append(env.state.drone.clone()), orig())[1]
        try:
            fn()
        finally:
            env._scan_snapshot = orig
        if snaps:                              # the snapshot the update read is the pose of before the step
            assert torch.equal(env.scan['pose'], snaps[-1])
        return len(snaps), env.backend.scan_updates - before
    act = torch.zeros(2, dtype=torch.float64)
    env = SB.env_of(p, 2, scan_obs=True)
    assert env.backend.scan_updates == 0                                # no launch at construction: no rays yet
    SC.check_cleared(env, 0)
    assert count(env, lambda: env.step(act)) == (1, 1)
    assert count(env, env.perceive) == (1, 1) and count(env, lambda: env.act(act)) == (0, 0)
    assert count(env, env._plugins_step) == (1, 1)
    assert count(env, lambda: env.closed_loop(1)) == (1, 1)
    assert env.scan['last_step'].tolist() == [4, 4]
    assert count(env, lambda: env.reset(torch.tensor([1, 0], dtype=torch.uint8))) == (0, 0)
    SC.check_cleared(env, 0)
    assert int(env.scan['last_step'][1]) == 4 and bool(env.ray_kind[1].any())
    log = []
    for name in ('closed_loop', 'scan_update'):
        fn = getattr(env.backend, name)
        setattr(env.backend, name, lambda *a, _n=name, _f=fn, **k: (log.append((_n, a[3] if _n == 'closed_loop' else None)), _f(*a, **k))[1])
    assert count(env, lambda: env._episode_steps(3)) == (3, 3)          # Primitive under CVM: its one-step persistent launch, three times
    assert log == [('closed_loop', 1), ('scan_update', None)] * 3
    ox = SB.env_of(AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'), 2, scan_obs=True, gaze='Oxford')
    assert count(ox, ox.policy_step) == (1, 1) and count(ox, lambda: ox.run_episodes(max_steps=3)) == (3, 3)
    nomove = SB.env_of(AC.params_of(pkg, 'Primitive-CVM', planner='NoMove'), 2, scan_obs=True, device_plugins=False, gaze=None)
    assert count(nomove, lambda: nomove.step(act)) == (1, 1) and 'scan' in nomove._result()[0]
    jp = AC.params_of(pkg, 'Jerk-CVM')
    jerk = SB.env_of(jp, 2, backend=SB.ScanJerkBackend(), scan_obs=True)
    assert count(jerk, lambda: jerk.step(act)) == (1, 1) and count(jerk, lambda: jerk._jerk_step(True)) == (1, 1)
    assert count(jerk, lambda: jerk._episode_steps(2)) == (2, 2)
    rvo = SB.env_of(AC.params_of(pkg, 'Primitive-RVO'), 2, scan_obs=True)
    assert count(rvo, lambda: rvo._episode_steps(2)) == (2, 2) and count(rvo, lambda: rvo.step(act)) == (1, 1)
    # the rays are the model's for the pose of before the step and the agents of behind it, whatever path moved the env
    for e_ in (env, ox, nomove, jerk, rvo):
        for e in range(2):
            assert int(e_.scan['last_step'][e]) == int(e_.state.counters[e, A.C_STEPS]) >= 1
            SC.check_against_model(e_, e)


def test_reset_and_refill_clear_the_channel_and_the_equal_step_count_trap(pkg):
    """a slot whose previous episode ended at step k is not skipped at step k of its next one"""
    p = AC.params_of(pkg, 'Primitive-CVM', planner='NoMove')
    env = SB.env_of(p, 2, scan_obs=True, device_plugins=False, gaze=None)
    act = torch.zeros(2, dtype=torch.float64)
    for _ in range(3):
        env.step(act)
    first = [t.clone() for t in (env.ray_end, env.ray_kind, env.scan['hit'])]
    assert env.scan['last_step'].tolist() == [3, 3]
    env.reset(torch.tensor([1, 0], dtype=torch.uint8))
    SC.check_cleared(env, 0)
    assert int(env.scan['last_step'][1]) == 3 and torch.equal(env.ray_end[1], first[0][1])
    env.state.drone[0, A.D_YAW] = 180.0                                 # the new episode looks elsewhere
    for t in range(3):
        env.step(act)
        assert int(env.scan['last_step'][0]) == t + 1
        SC.check_against_model(env, 0)
    assert not torch.equal(env.ray_end[0], first[0][0])                 # step 3 of the new episode: its own rays, not the old step 3's
    env.reset()
    SC.check_cleared(env, 0), SC.check_cleared(env, 1)
    # the masked fills of a refill (stream_episodes) and the item list of an action stream's restore name the same buffers
    env.step(act)
    env._scan_zero(torch.tensor([0, 1], dtype=torch.uint8))
    SC.check_cleared(env, 1)
    assert int(env.scan['last_step'][0]) == 1
    from drone2d_amd.action_stream import restore_items
    names = [it.name for it in restore_items(env)]
    assert [n for n in names if n.startswith('scan.')] == ['scan.' + n for n in A.SCAN_OUTPUTS]


def test_without_the_keyword_nothing_is_added(pkg):
    env = SB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1)
    assert env.scan_obs is False and env.scan is None
    env.step(torch.zeros(1, dtype=torch.float64))
    assert sorted(env._result()[0]) == ['local_map', 'swep_map', 'yaw_angle'] and env.backend.scan_updates == 0
    for name in ('ray_end', 'ray_kind', 'ray_hits'):
        with pytest.raises(RuntimeError, match='scan_obs=True'):
            getattr(env, name)


def test_the_refusals(pkg):
    from stepped_backend import SteppedOracleBackend
    p = AC.params_of(pkg, 'Primitive-CVM')
    with pytest.raises(NotImplementedError, match=r'oracle\+rvo_host\+live has no per-ray scan launch \(include/d2d_scan\.h'):
        SB.env_of(p, 1, backend=SteppedOracleBackend(), scan_obs=True)
    env = SB.env_of(p, 1, scan_obs=True)
    with pytest.raises(NotImplementedError, match=r'closed_loop\(\): scan_obs=True.*action_stream\(\) / policy_step\(\) / run_episodes\(\)'):
        env.closed_loop(2)
    with pytest.raises(NotImplementedError, match=r'closed_loop\(\): scan_obs=True'):
        env.closed_loop(1, auto_reset=True)
    with pytest.raises(NotImplementedError, match=r'rollout\(\): scan_obs=True.*step\(\) / action_stream\(\) / policy_step\(\) / run_episodes\(\)'):
        env.rollout(torch.zeros((2, 1), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------- the host build
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    lib = host_build.shared('scan_host.c', tmp_path_factory.mktemp('scan'), 'libscan_host.so')
    P = C.POINTER
    lib.scan_host_update.argtypes = [P(A.Cfg), P(A.State), P(A.Scan)]
    lib.scan_host_check.argtypes = [P(A.Cfg), P(A.State), P(A.Scan), C.c_char_p, C.c_int]
    lib.scan_host_cell.argtypes = [C.c_double, C.c_double, C.c_int]
    lib.scan_host_positive_angle.argtypes = [C.c_double]
    lib.scan_host_positive_angle.restype = C.c_double
    return lib


def _handmade_env(pkg, k):
    p, layout = SC.handmade_params(pkg, k)
    env = SB.env_of(p, 16, scan_obs=True, planner=p.planner, device_plugins=False, gaze=None, grid_layout=layout)
    size, n, _ = SC.HANDMADE[k]
    assert (env.cfg.W, env.cfg.H, env.cfg.N, env.cfg.grid_tile) == (size[0] // 10, size[1] // 10, n, 16 if layout == 'tiled' else 0)
    return env


def _special_env(pkg, name):
    p, layout = SC.SPECIAL[name][0](pkg)
    env = SB.env_of(p, 16, scan_obs=True, planner=p.planner, device_plugins=False, gaze=None, grid_layout=layout)
    assert (env.cfg.W, env.cfg.H, env.cfg.N, env._scan.hit_words) == (50, 50, p.agent_number, (p.agent_number + 31) // 32)
    return env


HANDMADE_ALONE = 2       # the finished env and the env with counter 0


@host_build.needs_fma('csrc/scan/d2d_scan.h restates a libm tan that fuses multiply-adds (-mfma)')
@pytest.mark.parametrize('k', list(range(len(SC.HANDMADE))) + list(SC.SPECIAL))
def test_the_host_build_against_the_model_on_the_handmade_poses(pkg, host, k):
    """... and on the crowd (63, 64, 65 and 72 candidates: the culled list below and at its capacity, and the fallback to every
    agent above it) and the ring at the cull bound, tests/scan_cases.SPECIAL"""
    if k in SC.SPECIAL:
        env = _special_env(pkg, k)
        alone, kinds = SC.run_special(env, k, lambda: host.scan_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._scan)))
        assert alone == 0 and sum(kinds) == 16 * env.cfg.R and kinds[2] > 0 and kinds[3] > 0
        return
    env = _handmade_env(pkg, k)

    def launch():
        assert host.scan_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._scan)) == 0
    alone, kinds = SC.run_handmade(env, launch)
    assert alone == HANDMADE_ALONE and kinds[0] >= 2 * env.cfg.R and kinds[1] > 0 and kinds[3] > 0
    assert (kinds[2] >= 2 * env.cfg.R) == (env.cfg.N >= 2)


@host_build.needs_fma('csrc/scan/d2d_scan.h restates a libm tan that fuses multiply-adds (-mfma)')
def test_the_host_build_replays_an_episode(pkg, host):
    """the recorded poses of the wide teleport episode through the C loop alone: the reference's rays at every step"""
    ep = SC.episode(3)
    env = SB.env_of(SC.params_of(pkg, ep), 1, scan_obs=True, **SC.env_kw(ep))
    launch = env.backend.scan_update
    env.backend.scan_update = lambda cfg, st, w: None                    # the env steps, the C loop scans
    try:
        for t in range(len(ep['action'])):
            env.state.drone[0, :3] = torch.from_numpy(ep['tele'][t].copy())
            env.step(torch.tensor([float(ep['action'][t])], dtype=torch.float64))
            assert host.scan_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._scan)) == 0
            SC.check_step(env, ep, t)
    finally:
        env.backend.scan_update = launch


@host_build.needs_fma('csrc/scan/d2d_scan.h restates a libm tan that fuses multiply-adds (-mfma)')
def test_the_host_build_under_the_sanitizers(pkg, host, tmp_path):
    """the handmade sets, the crowd and the ring through a stand-alone program built with AddressSanitizer and UBSan, on exactly
    sized heap arrays: every index the loop forms -- the grid in either layout, the last ray's last hit word, the candidate list at
    its capacity and the agents' planes behind the fallback -- stays inside its array"""
    import struct
    import subprocess
    records = []
    for k in range(len(SC.HANDMADE)):
        env = _handmade_env(pkg, k)
        SC.run_handmade(env, lambda: host.scan_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._scan)), records)
    for name in SC.SPECIAL:
        env = _special_env(pkg, name)
        SC.run_special(env, name, lambda: host.scan_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._scan)), records)
    assert len(records) == len(SC.HANDMADE) + 2
    path = tmp_path / 'records.bin'
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(records)))
        for r in records:
            c = r['cfg']
            f.write(struct.pack('<8i6d', c.B, c.N, c.W, c.H, c.R, c.grid_tile, r['hit_words'], 0, c.scale, c.W_px, c.H_px, c.ray_off0, c.ray_dth,
                                c.depth))
            for a in (r['agents'], r['counters'], r['gt'], r['pose']):
                f.write(np.ascontiguousarray(a).tobytes())
            for k in ('end', 'kind', 'hit', 'obs', 'last_step'):
                f.write(np.ascontiguousarray(r['before'][k]).tobytes())
            for k in ('end', 'kind', 'hit', 'obs', 'last_step'):
                f.write(np.ascontiguousarray(r['want'][k]).tobytes())
    exe = host_build.sanitized(['scan_host.c', 'scan_host_main.c'], tmp_path, 'scan_host_san')
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


def test_the_cell_and_the_angle_are_pythons(host):
    rs = np.random.RandomState(1)
    vs = np.concatenate([rs.uniform(0, 500, 4000), np.arange(0, 53) * 10.0, np.nextafter(np.arange(1, 51) * 10.0, 0), [0.3 * 3 * 100, 1e300]])
    for s in (10.0, 3.0, 2.5):
        for v in vs:
            assert host.scan_host_cell(v, s, 50) == int(min(max(v // s, 0), 49)), (v, s)
    assert host.scan_host_cell(float('nan'), 10.0, 50) == 0
    for a in np.concatenate([rs.uniform(-20, 20, 4000), [0.0, math.pi * 2, -math.pi * 2, math.pi * 4, 7 * math.pi / 4]]):
        assert host.scan_host_positive_angle(float(a)) == SN.positive_angle(float(a)), a


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_the_mirror_and_the_built_library_without_a_gpu(pkg, host):
    from drone2d_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'd2d_scan.h')).read()
    assert re.findall(r'^(?:int|const char \*)\s*(d2d_scan_\w+)\(', header, re.M) == ['d2d_scan_version', 'd2d_scan_last_error', 'd2d_scan_update']
    body = re.search(r'typedef struct d2d_scan \{(.*?)\} d2d_scan;', header, re.S).group(1)
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+)(?:,\s*(\w+))?;', body, re.M)
    names = [n for _, a, b in fields for n in (a, b) if n]
    assert tuple(names) == tuple(n for n, _ in A.Scan._fields_)
    types = {n: t for t, a, b in fields for n in (a, b) if n}
    for n, ct in A.Scan._fields_:
        assert ct is (C.c_void_p if n in A.SCAN_POINTERS else {'int32_t': C.c_int32}[types[n]]), n
    assert set(A.SCAN_OUTPUTS) | {'pose'} == set(A.SCAN_POINTERS)
    assert int(re.search(r'#define\s+D2D_SCAN_VERSION\s+(\d+)', header).group(1)) == A.D2D_SCAN_VERSION == host.scan_host_version()
    assert host.scan_host_struct_bytes() == C.sizeof(A.Scan)
    d2d = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert 'scan_update' not in d2d and 'd2d_scan' not in d2d
    # the built library: its version, and every refusal comes before a launch, so this runs without a GPU
    lib, fn = _lib.load_scan_library()
    assert fn['version']() == A.D2D_SCAN_VERSION and sorted(fn) == ['last_error', 'update', 'version']
    err = lambda: fn['last_error']().decode()     # noqa: E731
    env = SB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1, scan_obs=True)
    cfg, st, good = env.cfg, env._st, env._scan
    up = lambda c, s, w: fn['update'](None if c is None else C.byref(c), None if s is None else C.byref(s), None if w is None else C.byref(w), None)   # noqa: E731
    assert up(None, st, good) == -1 and up(cfg, None, good) == -1 and up(cfg, st, None) == -1 and 'NULL' in err()
    assert up(A.Cfg(), st, good) == -2 and 'ABI' in err()
    assert up(cfg, A.State(), good) == -1 and err() == 'd2d_scan_update: agents, gt or counters is NULL'
    for name in A.SCAN_POINTERS:
        bad = A.Scan.from_buffer_copy(good)
        setattr(bad, name, None)
        assert up(cfg, st, bad) == -1 and err() == 'd2d_scan_update: a scan buffer is NULL', name
    import copy
    big = copy.copy(cfg)
    big.W, big.H = 32767 * 3, 32767
    assert up(big, st, good) == -4 and '32-bit indices' in err()
    why = C.create_string_buffer(256)
    assert host.scan_host_check(C.byref(big), C.byref(st), C.byref(good), why, 256) == -4 and why.value.decode() == err()
    many = copy.copy(cfg)
    many.R = 1 << 30
    wide = A.Scan.from_buffer_copy(good)
    wide.hit_words = 4
    assert up(many, st, wide) == -4 and 'R * hit_words' in err()
    short = A.Scan.from_buffer_copy(good)
    short.hit_words = 0
    assert up(cfg, st, short) == -1 and 'hit_words' in err()
    crowd = copy.copy(cfg)
    crowd.N = 33
    assert up(crowd, st, good) == -1 and 'hit_words' in err()
    unit = copy.copy(cfg)
    unit.scale = 1.0
    assert up(unit, st, good) == -1 and 'scale > 1' in err()
    none = copy.copy(cfg)
    none.B = 0
    assert up(none, st, good) == 0


# ---------------------------------------------------------------------------------------------------------------- the facade
def test_the_facades_rays(pkg):
    """Drone2DEnv2(..., rays=True): {} before the first step, then the reference's records of the teleport episode, built when read;
    the default keeps the constant {}"""
    from drone2d_amd import env as envmod
    ep = SC.episode(0)
    p = SC.params_of(pkg, ep)
    plain = envmod.Drone2DEnv2(p, backend=SB.ScanOracleBackend())
    assert plain.drone.rays == {} and plain._vec.scan is None
    plain.step(0.0)
    assert plain.drone.rays == {} and plain._backend.scan_updates == 0
    e = envmod.Drone2DEnv2(p, backend=SB.ScanOracleBackend(), rays=True)
    assert e.drone.rays == {} and e._vec.scan_obs
    N = e._vec.N
    for t in range(10):
        e.drone.x, e.drone.y, e.drone.yaw = (float(v) for v in ep['tele'][t])
        e.step(float(ep['action'][t]))
        pulls = e._pull_count
        rays = e.drone.rays
        assert e.drone.rays is rays and e._pull_count == pulls              # built once per step, and only when read
        assert isinstance(rays, list) and len(rays) == 50 and sorted(rays[0]) == ['coords', 'hit_list', 'wall']
        for i, ray in enumerate(rays):
            assert tuple(ray['coords']) == tuple(ep['coords'][t, i]), (t, i)
            assert ray['hit_list'].dtype == torch.int8 and ray['hit_list'].tolist() == SC.unpack(ep['hit'][t, i], N).tolist(), (t, i)
            raw = int(ep['wall'][t, i])
            assert ray['wall'] == (2 if raw == 3 and ep['kind'][t, i] == 3 else raw), (t, i)
        hit = np.zeros(N, dtype=np.uint8)          # what tests/golden/make_golden.py does with them
        for ray in rays:
            hit |= ray['hit_list'].numpy().astype(np.uint8)
        assert np.array_equal(hit, e._mirror['hit'])
    assert e.reset() == {} and e.drone.rays == {}
