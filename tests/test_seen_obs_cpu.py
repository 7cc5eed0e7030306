"""seen_obs=True without a GPU (include/d2d_seen.h through tests/seen_backend.py, whose launch is the numpy model of
tests/seen_model.py): the reference's recorded maps step for step, streams with and without the channel, every stepping path, the
refusals, the host build of csrc/seen/d2d_seen.h against the model on the handmade poses, and the header against its ctypes mirror.
Every comparison is exact equality: integers, and the bit patterns of floats."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import action_stream_backend as AB
import action_stream_cases as AC
import host_build
import seen_backend as SB
import seen_cases as SC
import seen_model as SN
from drone2d_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(env, action):
    env._set_action(action)
    env._plugins_step()


def test_the_fixture_covers_what_it_is_for():
    reseen, inside, never = SC.coverage()
    assert reseen >= 100 and inside >= 20 and never >= 1, (reseen, inside, never)
    assert os.path.getsize(SC.PATH) < 200 * 1000
    cfgs = [SC.episode(i)['cfg'] for i in range(SC.EPISODES)]
    assert sum('seed' in c for c in cfgs) == 2 and sum(c.get('drone_view_range') == 120 for c in cfgs) == 1
    assert sum(c.get('init_pos') == [250, 250] and c.get('target_list') == [[60, 440]] for c in cfgs) == 1


@pytest.mark.parametrize('i', range(SC.EPISODES))
def test_the_recorded_episodes_through_the_env(pkg, i):
    """map, crop and refreshed of every step, and of step 0 before any step"""
    ep = SC.episode(i)
    env = SB.env_of(SC.params_of(pkg, ep), 1, seen_obs=True)
    assert SC.replay(env, ep, _step) == len(ep['action'])
    # the terminal step moved the counter, so the map was updated once more; then the env is finished and nothing moves
    T = len(ep['action'])
    assert int(env.seen['last_call'][0]) == T + 1
    keep = [t.clone() for t in (env.seen_calls, env.seen['obs'], env.refreshed, env.seen['last_call'])]
    _step(env, torch.zeros(1, dtype=torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(keep, (env.seen_calls, env.seen['obs'], env.refreshed, env.seen['last_call'])))


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_a_stream_with_and_without_the_channel(pkg, cell):
    p = AC.params_of(pkg, cell)
    cls = SB.SeenTurnJerkBackend if p.planner == 'Jerk_Primitive' else SB.SeenTurnBackend
    make = lambda q, n, seen: AB.env_of(q, n, backend=cls().of(q), seen_obs=True) if seen else AB.env_of(q, n)      # noqa: E731
    refills, frozen = SC.stream_pair(make, p, 3, 9)
    assert refills == 9 - 3 and frozen > 0


def test_stream_episodes_refills_through_the_masked_fills(pkg):
    """stream_episodes() (a policy of the device's) rebuilds a slot through _refill_rest: a refilled slot shows the call-1 map"""
    p = AC.params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    env = AB.env_of(p, 2, backend=SB.SeenTurnBackend().of(p), seen_obs=True, gaze='Rotating')
    rounds = 0
    for finished, refill in env.stream_rounds(5, refill_every=8):
        for e in np.nonzero(refill.numpy())[0]:
            SC.check_call_1(env, int(e))
            rounds += 1
    assert rounds >= 3 and int((env.stream_rows[:, 0] > 0).sum()) == 5


def test_every_stepping_path_queues_one_update_per_step(pkg):
    p = AC.params_of(pkg, 'Primitive-CVM')

    def count(env, fn):
        before = env.backend.seen_updates
        fn()
        return env.backend.seen_updates - before
    act = torch.zeros(2, dtype=torch.float64)
    env = SB.env_of(p, 2, seen_obs=True)
    assert env.backend.seen_updates == 1                                # call 1 at construction
    assert count(env, lambda: env.step(act)) == 1
    assert count(env, env.perceive) == 0 and count(env, lambda: env.act(act)) == 1
    assert count(env, env._plugins_step) == 1
    assert count(env, lambda: env.reset(torch.tensor([1, 0], dtype=torch.uint8))) == 1
    assert env.seen['last_call'].tolist() == [1, 4] and int(env.seen_calls[0].max()) == 1 and int(env.seen_calls[1].max()) == 4
    SC.check_call_1(env, 0)
    log = []
    for name in ('closed_loop', 'seen_update'):
        fn = getattr(env.backend, name)
        setattr(env.backend, name, lambda *a, _n=name, _f=fn, **k: (log.append((_n, a[3] if _n == 'closed_loop' else None)), _f(*a, **k))[1])
    env._episode_steps(3)                                               # Primitive under CVM: its one-step persistent launch, three times
    assert log == [('closed_loop', 1), ('seen_update', None)] * 3
    ox = SB.env_of(AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'), 2, seen_obs=True, gaze='Oxford')
    assert count(ox, ox.policy_step) == 1 and count(ox, lambda: ox.run_episodes(max_steps=3)) == 3
    nomove = SB.env_of(AC.params_of(pkg, 'Primitive-CVM', planner='NoMove'), 2, seen_obs=True, device_plugins=False, gaze=None)
    assert count(nomove, lambda: nomove.step(act)) == 1 and 'age_map' in nomove._result()[0]
    jp = AC.params_of(pkg, 'Jerk-CVM')
    jerk = SB.env_of(jp, 2, backend=SB.SeenJerkBackend(), seen_obs=True)
    assert count(jerk, lambda: jerk.step(act)) == 1 and count(jerk, lambda: jerk._jerk_step(True)) == 1
    assert count(jerk, lambda: jerk._episode_steps(2)) == 2
    # the update is the model's for the pose the env is in, whatever path moved it
    for e_ in (env, ox, nomove, jerk):
        for e in range(2):
            d, call = e_.state.drone[e].numpy(), int(e_.state.counters[e, A.C_STEPS]) + 1
            view = SN.view_map(d[0], d[1], d[2], e_.cfg.W, e_.cfg.H, e_.cfg.scale, float(e_.cfg.depth), e_.params.drone_view_range)
            assert int(e_.seen['last_call'][e]) == call and np.array_equal(e_.seen_calls[e].numpy() == call, view)


def test_without_the_keyword_nothing_is_added(pkg):
    env = SB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1)
    assert env.seen_obs is False and env.seen is None and env.backend.seen_updates == 0
    env.step(torch.zeros(1, dtype=torch.float64))
    assert sorted(env._result()[0]) == ['local_map', 'swep_map', 'yaw_angle'] and env.backend.seen_updates == 0
    for name in ('seen_calls', 'seen_age', 'refreshed'):
        with pytest.raises(RuntimeError, match='seen_obs=True'):
            getattr(env, name)


def test_the_refusals(pkg):
    from stepped_backend import SteppedOracleBackend
    p = AC.params_of(pkg, 'Primitive-CVM')
    with pytest.raises(NotImplementedError, match=r'oracle\+rvo_host\+live has no time-since-observed launch \(include/d2d_seen\.h'):
        SB.env_of(p, 1, backend=SteppedOracleBackend(), seen_obs=True)
    env = SB.env_of(p, 1, seen_obs=True)
    with pytest.raises(NotImplementedError, match=r'closed_loop\(\): seen_obs=True.*action_stream\(\) / policy_step\(\) / run_episodes\(\)'):
        env.closed_loop(1)
    with pytest.raises(NotImplementedError, match=r'rollout\(\): seen_obs=True'):
        env.rollout(torch.zeros((2, 1), dtype=torch.float64))
    from drone2d_amd.device_plugins import acos_window
    import math
    with pytest.raises(NotImplementedError) as want:
        acos_window(math.radians(180 / 2))
    with pytest.raises(NotImplementedError) as got:
        SB.env_of(AC.params_of(pkg, 'Primitive-CVM', drone_view_range=180), 1, seen_obs=True)
    assert str(got.value) == str(want.value) and '64-double decision window' in str(got.value)


# ---------------------------------------------------------------------------------------------------------------- the host build
@pytest.fixture(scope='module')
def host(tmp_path_factory):
    lib = host_build.shared('seen_host.c', tmp_path_factory.mktemp('seen'), 'libseen_host.so')
    P = C.POINTER
    lib.seen_host_update.argtypes = [P(A.Cfg), P(A.State), P(A.Seen)]
    lib.seen_host_check.argtypes = [P(A.Cfg), P(A.State), P(A.Seen), C.c_char_p, C.c_int]
    lib.seen_host_cell.argtypes = [C.c_double, C.c_double, C.c_int]
    return lib


@host_build.needs_fma('csrc/seen/d2d_seen.h takes the floor of a quotient with a fused remainder (-mfma)')
@pytest.mark.parametrize('k', range(5))
def test_the_host_build_against_the_model_on_the_handmade_poses(pkg, host, k):
    p, view_range, poses = SC.handmade_sets(pkg)[k]
    env = SB.env_of(p, len(poses), seen_obs=True, planner=p.planner, device_plugins=False, gaze=None)
    assert (env.cfg.W, env.cfg.H) == [(50, 50), (30, 20), (20, 30), (50, 50), (50, 50)][k]

    def launch():
        assert host.seen_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._seen)) == 0
    alone, marked, fresh = SC.run_handmade(env, view_range, poses, launch)
    assert alone == (2 if k == 0 else 0) and marked > 5 * len(poses) and 0 < fresh < marked     # (a 60 degree sector of radius 4.5 cells: 10)


@host_build.needs_fma('csrc/seen/d2d_seen.h takes the floor of a quotient with a fused remainder (-mfma)')
def test_the_host_build_replays_an_episode(pkg, host):
    """the recorded poses of the interior-start episode through the C loop alone: the reference's map at every call"""
    ep = SC.episode(3)
    env = SB.env_of(SC.params_of(pkg, ep), 1, seen_obs=True)
    for n in ('seen', 'last_call'):
        env.seen[n].zero_()
    for t, pose in enumerate(ep['pose']):
        env.state.drone[0, :3] = torch.from_numpy(pose)
        env.state.counters[0, A.C_STEPS] = t
        assert host.seen_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._seen)) == 0
        assert np.array_equal(SC.bits(env.seen_age[0].numpy()), SC.bits(ep['map'][t])), t


def test_the_host_build_under_the_sanitizers(pkg, host, tmp_path):
    """the handmade sets through a stand-alone program built with AddressSanitizer and UBSan, on exactly sized heap arrays: every
    index the loop forms -- the view box, the crop window, the table -- stays inside its array"""
    import struct
    import subprocess
    records = []
    for p, view_range, poses in SC.handmade_sets(pkg):
        env = SB.env_of(p, len(poses), seen_obs=True, planner=p.planner, device_plugins=False, gaze=None)
        SC.run_handmade(env, view_range, poses, lambda: host.seen_host_update(C.byref(env.cfg), C.byref(env._st), C.byref(env._seen)), records)
    path = tmp_path / 'records.bin'
    with open(path, 'wb') as f:
        f.write(struct.pack('<i', len(records)))
        for r in records:
            c = r['cfg']
            f.write(struct.pack('<6i2dqQ', c.B, c.W, c.H, c.L, r['tab'].shape[1], 0, c.scale, c.depth, r['key_lo'], r['mask']))
            for k in ('drone', 'counters', 'seen', 'last_call', 'refreshed', 'obs', 'tab'):
                f.write(np.ascontiguousarray(r[k]).tobytes())
            for k in ('seen', 'last_call', 'refreshed', 'obs'):
                f.write(np.ascontiguousarray(r['want'][k]).tobytes())
    exe = host_build.sanitized(['seen_host.c', 'seen_host_main.c'], tmp_path, 'seen_host_san')
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]


def test_the_cell_of_a_coordinate_is_pythons_floor_division(host):
    rs = np.random.RandomState(1)
    vs = np.concatenate([rs.uniform(-30, 530, 4000), np.arange(-3, 53) * 10.0, np.nextafter(np.arange(1, 51) * 10.0, 0), [0.3 * 3 * 100, 1e300, -1e300]])
    for s in (10.0, 3.0, 0.1):
        for v in vs:
            assert host.seen_host_cell(v, s, 50) == int(min(max(v // s, -2), 51)), (v, s)
    assert host.seen_host_cell(float('nan'), 10.0, 50) == -2


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_the_mirror_and_the_built_library_without_a_gpu(pkg, host):
    from drone2d_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'd2d_seen.h')).read()
    assert re.findall(r'^(?:int|const char \*)\s*(d2d_seen_\w+)\(', header, re.M) == ['d2d_seen_version', 'd2d_seen_last_error', 'd2d_seen_update']
    body = re.search(r'typedef struct d2d_seen \{(.*?)\} d2d_seen;', header, re.S).group(1)
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+);', body, re.M)
    assert tuple(n for _, n in fields) == tuple(n for n, _ in A.Seen._fields_)
    ctype = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64}
    for (t, n), (m, ct) in zip(fields, A.Seen._fields_):
        assert ct is (C.c_void_p if n in A.SEEN_POINTERS else ctype[t]), n
    assert set(A.SEEN_BUFFERS) | {'tab'} == set(A.SEEN_POINTERS)
    assert int(re.search(r'#define\s+D2D_SEEN_VERSION\s+(\d+)', header).group(1)) == A.D2D_SEEN_VERSION == host.seen_host_version()
    assert host.seen_host_struct_bytes() == C.sizeof(A.Seen)
    d2d = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert 'seen_update' not in d2d and 'd2d_seen' not in d2d
    # the built library: its version, and every refusal comes before a launch, so this runs without a GPU
    lib, fn = _lib.load_seen_library()
    assert fn['version']() == A.D2D_SEEN_VERSION and sorted(fn) == ['last_error', 'update', 'version']
    err = lambda: fn['last_error']().decode()     # noqa: E731
    env = SB.env_of(AC.params_of(pkg, 'Primitive-CVM'), 1, seen_obs=True)
    cfg, st, good = env.cfg, env._st, env._seen
    up = lambda c, s, w: fn['update'](None if c is None else C.byref(c), None if s is None else C.byref(s), None if w is None else C.byref(w), None)   # noqa: E731
    assert up(None, st, good) == -1 and up(cfg, None, good) == -1 and up(cfg, st, None) == -1 and 'NULL' in err()
    assert up(A.Cfg(), st, good) == -2 and 'ABI' in err()
    assert up(cfg, A.State(), good) == -1 and err() == 'd2d_seen_update: drone or counters is NULL'
    for name in A.SEEN_POINTERS:
        bad = A.Seen.from_buffer_copy(good)
        setattr(bad, name, None)
        assert up(cfg, st, bad) == -1 and err() == 'd2d_seen_update: a seen buffer is NULL', name
    import copy
    big = copy.copy(cfg)
    big.W, big.H = 32767, 32767 * 3
    assert up(big, st, good) == -4 and '32-bit cell indices' in err()
    why = C.create_string_buffer(256)
    assert host.seen_host_check(C.byref(big), C.byref(st), C.byref(good), why, 256) == -4 and why.value.decode() == err()
    short = A.Seen.from_buffer_copy(good)
    short.tab_len = 1
    assert up(cfg, st, short) == -1
    none = copy.copy(cfg)
    none.B = 0
    assert up(none, st, good) == 0
