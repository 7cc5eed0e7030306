"""Action streams without a GPU (VecDrone2DEnv.action_stream, action_stream.ActionStream) on the model backends of
tests/action_stream_backend.py: include/d2d_worlds_turn.h against its ctypes mirror, the item list of d2d_stream_restore against a
hand-written list per cell, the refusals, the turn against the existing assign model for scripted done flags, the terminal state, the
rows against the reference batch in all four cells, and the scalar item logic of the restore in a stand-alone sanitized program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import action_stream_backend as AB
import action_stream_cases as AC
import host_build
import stream_model as SM
from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'd2d_worlds_turn.h')).read()


def make(params, n, **kw):
    return AB.env_of(params, n, **kw)


# ---------------------------------------------------------------------------------------------------------------- the ABI
class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


KINDS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'double': C.c_double}


def argtypes_of(args):
    out = []
    for a in args.replace('\n', ' ').strip().split(','):
        words = a.replace('*', ' * ').split()
        if '*' in words:
            out.append(C.POINTER(A.State) if 'd2d_state' in words else C.c_void_p)
        else:
            out.append(KINDS[words[0]])
    return out


def test_the_header_against_the_mirror():
    declared = dict(re.findall(r'^int\s*(d2d_\w+)\(([^;]*)\);', HEADER, re.M))
    assert sorted(declared) == sorted('d2d_' + n for n in A.TURN_ENTRY_POINTS) == ['d2d_stream_explored', 'd2d_stream_restore']
    bound = A.bind_worlds_turn(Recorder())
    for name, args in declared.items():
        fn = bound[name[len('d2d_'):]]
        assert fn.argtypes == argtypes_of(args) and fn.restype is C.c_int, name
    # the record: field order, types and size
    body = re.search(r'typedef struct d2d_restore_item \{(.*?)\} d2d_restore_item;', HEADER, re.S).group(1)
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);', body, re.M)
    want = [(n, C.c_void_p if star else KINDS[t]) for t, star, n in fields]
    assert want == list(A.RestoreItem._fields_)
    assert [n for n, _ in want] == ['dst', 'src', 'dst_stride', 'src_stride', 'dst_off', 'src_off', 'bytes', 'kind', 'reserved']
    assert C.sizeof(A.RestoreItem) == 64 and A.RestoreItem.bytes.offset == 48 and A.RestoreItem.kind.offset == 56
    define = lambda n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', HEADER).group(1), 0)   # noqa: E731
    for name in ('MAX_ITEMS', 'ZERO', 'COPY', 'PARTS'):
        assert define('D2D_RESTORE_' + name) == getattr(A, 'RESTORE_' + name), name
    assert A.RESTORE_MAX_ITEMS == 32 and 'D2D_WORLDS_VERSION 1' not in HEADER and A.D2D_WORLDS_VERSION == 1
    assert not set(bound) & set(A.bind_worlds_stream(Recorder())) and not set(bound) & set(A.bind_worlds(Recorder()))


@pytest.mark.parametrize('missing', A.TURN_ENTRY_POINTS)
def test_a_library_without_either_symbol_announces_no_action_stream(missing):
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_' + missing:
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    hb = _lib.HipBackend.__new__(_lib.HipBackend)
    hb.sfn = dict(A.bind_worlds_stream(Old()), **A.bind_worlds_turn(Old()))
    assert hb.supports_action_stream is False and hb.supports_episode_stream is True
    with pytest.raises(_lib.D2DError, match='d2d_worlds_turn.h'):
        z = torch.zeros(2, dtype=torch.uint8)
        getattr(hb, missing)(*((z, 0, z) if missing == 'stream_restore' else (A.Cfg(), A.State(), z)))
    hb.sfn = A.bind_worlds_turn(Recorder())
    assert hb.supports_action_stream is True


def test_the_built_library_exports_them_and_refuses_bad_arguments_without_a_gpu():
    lib, wfn = _lib.load_worlds_library()
    fn = A.bind_worlds_turn(lib)
    assert sorted(fn) == sorted(A.TURN_ENTRY_POINTS) and wfn['version']() == 1
    one, st, err = C.c_void_p(8), A.State(), wfn['last_error']          # never dereferenced: every call below is refused first
    assert fn['stream_restore'](one, 33, one, 2, None) == -1 and b'MAX_ITEMS' in err()
    assert fn['stream_restore'](one, -1, one, 2, None) == -1 and fn['stream_restore'](one, 1, one, -2, None) == -1
    assert fn['stream_restore'](None, 1, one, 2, None) == -1 and b'NULL' in err()
    assert fn['stream_restore'](one, 1, None, 2, None) == -1 and b'NULL' in err()
    assert fn['stream_restore'](C.c_void_p(12), 1, one, 2, None) == -1 and b'aligned' in err()
    assert fn['stream_restore'](one, 1, one, 2 ** 31 - 1, None) == -4
    assert fn['stream_restore'](None, 0, None, 2, None) == 0 and fn['stream_restore'](None, 3, None, 0, None) == 0
    assert fn['stream_explored'](C.byref(st), 2, 50, 50, 8, one, None) == -1 and b'grid_tile' in err()
    assert fn['stream_explored'](C.byref(st), 2, 0, 50, 0, one, None) == -1
    assert fn['stream_explored'](C.byref(st), 2, 50, 50, 0, one, None) == -1 and b'NULL' in err()
    assert fn['stream_explored'](C.byref(st), 2, 50, 50, 0, None, None) == -1 and b'NULL' in err()
    assert fn['stream_explored'](C.byref(st), 0, 50, 50, 0, None, None) == 0


def test_the_scalar_item_logic_under_a_sanitizer(tmp_path):
    """csrc/worlds/d2d_restore.h, the text the kernel runs per thread, in a stand-alone program with ASan and UBSan: every workgroup and
    thread over heap buffers that end with the last range"""
    exe = host_build.sanitized(['restore_host_main.c'], tmp_path, 'restore_host')
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and 'restore_host ok' in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- the item list
Z, CP = A.RESTORE_ZERO, A.RESTORE_COPY
STATIC = dict(static_map='maps/obstacle_map.npy', agent_number=10)


def expected_items(cell, N, k, L, traj_cap, node_cap, hash_cap, noise):
    """(name, kind, dst_off, bytes, src_off) per item, written out by hand from VecDrone2DEnv._refill_rest"""
    out = [('plan_ok', Z, 0, 1, 0), ('wp_valid', Z, 0, 1, 0), ('wp', Z, 0, 48, 0), ('hit', Z, 0, N, 0), ('newly', Z, 0, 4, 0),
           ('obs_local', Z, 0, L * L, 0), ('obs_yaw', Z, 0, 4, 0)]
    if noise:
        out.append(('rng_draws', Z, 0, N * 16, 0))
    out.append(('action', Z, 0, 8, 0))
    if 'RVO' in cell:
        out += [('agent_vel.x[:k]', Z, 0, 8 * k, 0), ('agent_vel.y[:k]', Z, 8 * N, 8 * k, 0)]
        if N > k:
            out += [('agent_vel.x[k:]', CP, 8 * k, 8 * (N - k), 8 * (A.A_VX * N + k)), ('agent_vel.y[k:]', CP, 8 * (N + k), 8 * (N - k), 8 * (A.A_VY * N + k))]
    if 'Primitive' in cell:
        out += [('plan_stat', Z, 0, 16, 0), ('traj', Z, 0, traj_cap * 32, 0), ('traj_box', Z, 0, ((traj_cap + 63) // 64) * 32, 0),
                ('nodes', Z, 0, node_cap * A.NODE_F * 8, 0), ('hash', Z, 0, hash_cap * 4, 0)]
    if 'RVO' in cell:
        out.append(('agent_vel_out', Z, 0, 16 * N, 0))
    if 'Jerk' in cell:
        out += [('jerk.choice', Z, 0, 4, 0), ('jerk.stat', Z, 0, 4, 0)]
    return out + [('explored_prev', Z, 0, 4, 0)]


@pytest.mark.parametrize('cell', list(AC.CELLS))
@pytest.mark.parametrize('static', [False, True], ids=['seeded-agents', 'static-map-agents'])
def test_the_item_list_names_what_refill_rest_touches(pkg, cell, static):
    from drone2d_amd import action_stream
    p = AC.params_of(pkg, cell, **dict(STATIC if static else {}, var_cam=2 if static else 0))
    env = make(p, 2)
    if static:                                 # the model backends draw no noise on the device: the stream's field is named all the same
        env.state.t['rng_draws'] = torch.zeros((2, env.cfg.N, 2), dtype=torch.float64)
    prev = torch.zeros(2, dtype=torch.int32)
    items = action_stream.restore_items(env, prev)
    N, k = env.cfg.N, min(p.agent_number, env.cfg.N)
    assert (N > k) == static and k == p.agent_number
    sc = env.plugins.scalars if env.plugins is not None else dict(traj_cap=0, node_cap=0, hash_cap=0)
    want = expected_items(cell, N, k, env.cfg.L, sc['traj_cap'], sc['node_cap'], sc['hash_cap'], static)
    assert [(i.name, i.kind, i.dst_off, i.bytes, i.src_off) for i in items] == want
    assert len(items) <= A.RESTORE_MAX_ITEMS
    by_name = {i.name: i for i in items}
    s = env.state
    assert by_name['obs_local'].dst is s.obs_local and by_name['action'].dst is s.action and by_name['explored_prev'].dst is prev
    if 'RVO' in cell:
        assert by_name['agent_vel.y[:k]'].dst is s.agent_vel and by_name['agent_vel_out'].dst is s.agent_vel_out
        if static:
            assert by_name['agent_vel.x[k:]'].src is s.agents and by_name['agent_vel.x[k:]'].dst is s.agent_vel
    if 'Primitive' in cell:
        assert by_name['nodes'].dst is env.plugins.t['nodes'] and by_name['nodes'].bytes >= 150000
    # packed: the records carry the tensors' addresses and row strides; a range that leaves its row is refused before any launch
    packed, n = action_stream.pack_items(items, 'cpu')
    recs = (A.RestoreItem * n).from_address(packed.data_ptr())
    for r, i in zip(recs, items):
        assert (r.dst, r.dst_stride, r.dst_off, r.bytes, r.kind) == (i.dst.data_ptr(), i.dst[0].numel() * i.dst.element_size(), i.dst_off, i.bytes, i.kind)
        assert (r.src, r.src_stride) == ((i.src.data_ptr(), i.src[0].numel() * i.src.element_size()) if i.src is not None else (None, 0))
    bad = items[0]._replace(bytes=2)
    with pytest.raises(ValueError, match='leave the slot'):
        action_stream.pack_items([bad], 'cpu')
    with pytest.raises(ValueError, match='at most 32'):
        action_stream.pack_items(items[:1] * 33, 'cpu')


@pytest.mark.parametrize('cell', ['Primitive-RVO', 'Jerk-RVO'])
def test_the_restore_is_refill_rest(pkg, cell):
    """two identical envs, stepped alike, get the same refill mask: one through _refill_rest(), the other through the item list and the
    masked resets.  Every tensor is equal afterwards (the model of d2d_stream_restore against the masked fills)"""
    from drone2d_amd import action_stream
    p = AC.params_of(pkg, cell, **STATIC)
    envs = [make(p, 4), make(p, 4)]
    act = torch.linspace(-1, 1, 4, dtype=torch.float64)
    for env in envs:
        for _ in range(3):
            AC.unmasked_step(env, act)
    refill = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    envs[0]._refill_rest(refill)
    prev = torch.full((4,), 7, dtype=torch.int32)
    items, n = action_stream.pack_items(action_stream.restore_items(envs[1], prev), 'cpu')
    envs[1].backend.stream_restore(items, n, refill)
    envs[1].reset_plugins(refill)
    assert prev.tolist() == [0, 7, 0, 7]
    for e in range(4):
        assert AC.differing(AC.tensors(envs[0], e), AC.tensors(envs[1], e)) == [], e
    assert bool(envs[1].state.agent_vel[0, :, 10:].ne(0).any()) and not bool(envs[1].state.agent_vel[0, :, :10].ne(0).any())
    assert bool(envs[1].state.obs_local[1].ne(0).any()) and not bool(envs[1].state.obs_local[0].ne(0).any())


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg, oracle):
    from drone2d_amd import vec_env
    p = AC.params_of(pkg, 'Primitive-CVM')
    kw = dict(planner='Primitive', device_plugins=True, gaze='external')
    # a policy the device evaluates: that is stream_episodes()'s env
    env = make(p, 2, gaze='Oxford')
    with pytest.raises(RuntimeError, match=r"action_stream\(\) needs device_plugins=True.*gaze='external'"):
        env.action_stream(4)
    env = AB.backend_for_params(p).attach(vec_env.VecDrone2DEnv(p, 2, device='cpu', backend=AB.backend_for_params(p), worlds='device'))
    with pytest.raises(RuntimeError, match=r'action_stream\(\) needs device_plugins=True'):
        env.action_stream(4)
    # a backend without the two launches
    half = AB.backend_for_params(p)
    half.supports_action_stream = False
    with pytest.raises(NotImplementedError, match='d2d_worlds_turn.h'):
        make(p, 2, backend=half).action_stream(4)
    # stream_episodes()'s own refusals, word for word: no device worlds / no refill launches, host-built worlds, set_noise() rows, the
    # caller's noise without a device stream, map ids past 2**32, an env that has been stepped, a second stream
    with pytest.raises(NotImplementedError, match='device world construction.*ExperimentBatch'):
        vec_env.VecDrone2DEnv(p, 2, backend=oracle, **kw).action_stream(4)
    with pytest.raises(NotImplementedError, match="stream_episodes\\(\\): the worlds of this env were built on the host.*worlds='device'"):
        make(p, 2, worlds=None).action_stream(4)
    q = AC.params_of(pkg, 'Primitive-CVM', var_cam=2)
    env = make(q, 2)
    with pytest.raises(NotImplementedError, match='supports_device_noise'):
        env.action_stream(4)
    env.set_noise(np.zeros((2, env.N, 2)))
    with pytest.raises(NotImplementedError, match=r'set_noise\(\) rows belong to the envs'):
        env.action_stream(4)
    with pytest.raises(ValueError, match=r'2\*\*32.*split'):
        make(AC.params_of(pkg, 'Primitive-CVM', map_id=2 ** 32 - 3), 2).action_stream(4)
    env = make(p, 2)
    env.step(np.zeros(2))
    with pytest.raises(RuntimeError, match='has been stepped.*new VecDrone2DEnv / EpisodeStream'):
        env.action_stream(4)
    env = make(p, 2)
    stream = env.action_stream(4)
    with pytest.raises(RuntimeError, match='streamed episodes already'):
        env.action_stream(4)
    with pytest.raises(RuntimeError, match='has streamed'):
        env.reset()
    # a table row that moves the cfg
    with pytest.raises(ValueError, match='drone_max_speed.*is per stream'):
        make(p, 2, backend=AB.backend_for_params(p, table=True)).action_stream(episodes=[AC.params_of(pkg, 'Primitive-CVM'), AC.params_of(pkg, 'Primitive-CVM', map_id=4, drone_max_speed=20)])
    # actions: [B] float64 on the device
    ok = torch.zeros(2, dtype=torch.float64)
    for bad, exc in ((torch.zeros(2, dtype=torch.float32), TypeError), (np.zeros(2), TypeError), ([0.0, 0.0], TypeError),
                     (torch.zeros(3, dtype=torch.float64), ValueError), (torch.zeros((2, 1), dtype=torch.float64), ValueError)):
        with pytest.raises(exc, match=r'ActionStream.step\(\)'):
            stream.step(bad)
    assert stream.env.steps_streamed == 0
    stream.step(ok)
    stream.close()
    with pytest.raises(RuntimeError, match='closed'):
        stream.step(ok)


def test_the_default_number_of_episodes(pkg):
    """num_episodes=None without a table: STREAM_MAX_EPISODES clipped to the map ids below 2**32 (the clipped form is small enough
    to allocate here)"""
    p = AC.params_of(pkg, 'Jerk-CVM', map_id=2 ** 32 - 7)
    stream = make(p, 2).action_stream()
    assert stream.num_episodes == 7 and tuple(stream.rows.shape) == (7, A.STREAM_ROW_F)
    assert min(A.STREAM_MAX_EPISODES, 2 ** 32 - 100) == A.STREAM_MAX_EPISODES
    stream.close()


# ---------------------------------------------------------------------------------------------------------------- the turn
def test_the_turn_hands_out_episodes_in_the_assign_models_order(pkg):
    """done flags are scripted between the calls (a slot is declared done by hand); after every call slot_episode, the refill bytes
    and counts are those of stream_model.assign run beside the stream, at refill_every 1 and 2"""
    p = AC.params_of(pkg, 'Jerk-CVM')
    script = [[], [1], [], [0, 3], [], [2], [1, 4], [], [0, 1, 2, 3, 4], [], [2], [], []]
    for every in (1, 2):
        B, m = 5, 11
        stream = make(p, B).action_stream(m, refill_every=every)
        env = stream.env
        slot, map_id, refill, counts = np.arange(B, dtype=np.int32), np.zeros(B, np.uint32), np.zeros(B, np.uint8), np.array([B, 0], np.int64)
        act = torch.zeros(B, dtype=torch.float64)
        since = 0
        for call, done_now in enumerate(script):
            for e in done_now:
                env.state.flags[e, A.F_DONE] = 1
            flags = env.state.flags.numpy().copy()
            steps_before = env.state.counters[:, A.C_STEPS].numpy().copy()
            if since >= every:
                SM.assign(flags, slot, map_id, refill, counts, m, p.map_id)
                since = 0
                turned = True
            else:
                turned = False
            obs, terms, done, info = stream.step(act)
            since += 1
            assert info['episode'].tolist() == slot.tolist(), (every, call)
            assert stream.counts.tolist() == counts.tolist(), (every, call)
            if turned:
                assert stream.refill.tolist() == refill.tolist(), (every, call)
                for e in np.nonzero(refill)[0]:            # a refilled slot has played the first step of its new world
                    assert int(info['steps'][e]) == 1 and not bool(done[e]) and bool(info['live'][e])
                    assert int(stream._up['map_id'][e]) == p.map_id + slot[e]
            live = np.array(info['live'].tolist())
            assert (env.state.counters[:, A.C_STEPS].numpy()[~live] == steps_before[~live]).all()      # a finished slot is left alone
            assert (np.array(info['steps'].tolist())[live] > 0).all()
        assert counts[0] == m and (slot == -1).sum() > 0
        stream.close()


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Jerk-RVO'])
def test_the_terminal_state_is_visible_until_the_next_call(pkg, cell):
    AC.check_terminal_state(make, pkg, cell)


@pytest.mark.parametrize('cell', ['Primitive-RVO', 'Jerk-RVO'])
def test_a_refilled_slot_is_a_fresh_env(pkg, cell):
    AC.check_refilled_slot_is_fresh(make, pkg, cell)


@pytest.mark.parametrize('cell', list(AC.CELLS))
def test_rows_do_not_depend_on_the_schedule_or_the_slot(pkg, cell):
    p = AC.params_of(pkg, cell)
    want = AC.reference_records(make, p)
    assert (want[:, A.STREAM_R_FLAG0] != 0).any() and (want[:, A.STREAM_R_FLAG0 + 2] != 0).any()      # a collision and a freeze
    for every in (1, 3):
        rows, calls, refills = AC.stream_rows(make, p, AC.SLOTS, AC.M, every)
        assert np.array_equal(rows, want), (every, rows.tolist(), want.tolist())
        assert refills.max() >= 2 and refills.sum() == AC.M - AC.SLOTS


@pytest.mark.parametrize('m', [3, 5])
def test_fewer_episodes_than_slots_and_as_many(pkg, m):
    p = AC.params_of(pkg, 'Jerk-CVM')
    want = AC.reference_records(make, p, m)
    rows, calls, refills = AC.stream_rows(make, p, AC.SLOTS, m, 1)
    assert np.array_equal(rows, want) and refills.sum() == 0 and calls <= AC.MAX_STEPS + 1


def test_the_table_form_against_the_device_gaze_stream(pkg):
    import table_model as TM
    from drone2d_amd import vec_env

    def env_of_worlds(p, slots, worlds):
        return AB.env_of(p, slots, backend=AB.backend_for_params(p, table=True), worlds=worlds)
    AC.check_table_form(pkg, TM.table_stream_of, env_of_worlds,
                        lambda plist: vec_env.build_worlds_device_of(plist, 'cpu', AB.backend_for_params(plist[0], table=True)))
