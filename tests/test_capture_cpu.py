"""capture.Capture without a GPU: the selection rule's model (tests/capture_model.py) on hand-made states, include/d2d_capture.h against
its ctypes binding, the PNG encoder, the refusals and the file names against the model backends of tests/capture_backend.py, the
record_img / NoControl rule of runner.EpisodeStream, and whole streams with a capture on the host."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import capture_backend as CB
import capture_model as CM
from drone2d_amd import _abi as A
from drone2d_amd import _lib, capture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'd2d_capture.h')).read()
SMALL = dict(planner='Jerk_Primitive', map_size=[200, 130], init_pos=[20, 20], target_list=[[180, 110]], agent_number=6, agent_radius=8,
             agent_max_speed=30, drone_max_speed=30, pillar_number=2, drone_view_depth=40, drone_view_range=120, max_flight_time=3, map_id=3)


# ---------------------------------------------------------------------------------------------------------------- the model
def state(rows):
    """(flags [B, 4], counters [B, 8], drone [B, 8]) from rows (collision, dead_lock, freezing, done, steps, sm)"""
    B = len(rows)
    flags, counters = np.zeros((B, 4), np.uint8), np.zeros((B, 8), np.int32)
    for e, (col, dead, frz, done, steps, sm) in enumerate(rows):
        flags[e] = (col, dead, frz, done)
        counters[e, CM.C_STEPS], counters[e, CM.C_SM] = steps, sm
    drone = np.arange(B * 8, dtype=np.float64).reshape(B, 8) + 0.25
    return flags, counters, drone


def test_the_kinds_precedence():
    # every condition set at once is static or dynamic by the collision byte; then dead_lock, freezing, goal, other
    assert CM.kind_of([1, 1, 1, 1], [9, 0, 1]) == CM.STATIC and CM.kind_of([2, 1, 1, 1], [9, 0, 1]) == CM.DYNAMIC
    assert CM.kind_of([0, 1, 1, 1], [9, 0, 1]) == CM.DEAD_LOCK and CM.kind_of([0, 0, 1, 1], [9, 0, 1]) == CM.FREEZING
    assert CM.kind_of([0, 0, 0, 1], [9, 0, 1]) == CM.GOAL and CM.kind_of([0, 0, 0, 1], [9, 0, 3]) == CM.OTHER
    assert CM.kind_of([3, 0, 0, 1], [9, 0, 0]) == CM.OTHER          # a collision byte that is neither 1 nor 2 is no collision
    assert CM.NAMES == A.CAPTURE_KIND_NAMES == capture.ALL_KINDS and CM.ALL == (1 << A.CAPTURE_KINDS) - 1
    assert [capture.kind_mask([n]) for n in CM.NAMES] == [1, 2, 4, 8, 16, 32] and capture.kind_mask('goal') == 16
    assert CM.row_kind([12, 1, 0, 0, 0, 0, 0, 99]) == CM.GOAL and CM.row_kind([12, 3, 0, 0, 2, 1, 1, 99]) == CM.DYNAMIC


def test_select_filters_and_writes_in_slot_order():
    rows = [(1, 0, 0, 1, 5, 3),     # 0 static, done
            (2, 0, 0, 0, 5, 3),     # 1 dynamic but not done
            (2, 0, 0, 1, 7, 3),     # 2 dynamic, done
            (0, 0, 1, 1, 9, 3),     # 3 freezing, done: not asked for
            (1, 0, 0, 1, 0, 3),     # 4 static, done, no step played: a world that hit the attempt cap
            (1, 0, 0, 1, 4, 3),     # 5 static, done, retired
            (1, 0, 0, 1, 6, 1)]     # 6 static (and at the goal), done
    f, c, d = state(rows)
    ep = np.array([10, 11, 12, 13, 14, -1, 16], np.int32)
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(5, 8)
    took = CM.select(f, c, d, ep, CM.mask('static', 'dynamic'), 5, 8, sel_slot, sel_dst, meta, pose, counts)
    assert took == [0, 2, 6] and sel_slot.tolist() == [0, 2, 6, -1, -1] and sel_dst.tolist() == [0, 1, 2, -1, -1]
    assert meta[:3].tolist() == [[10, 1, 5, 0], [12, 2, 7, 2], [16, 1, 6, 6]] and (meta[3:] == -7).all()
    assert pose[:3].tolist() == [d[0, :3].tolist(), d[2, :3].tolist(), d[6, :3].tolist()] and (pose[3:] == -7).all()
    assert counts.tolist() == [3, 0, 3]
    # no slot_episode: every done slot, episode = slot; the retired slot 5 counts again, the one without a step still does not
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(7, 8)
    assert CM.select(f, c, d, None, CM.ALL, 7, 8, sel_slot, sel_dst, meta, pose, counts) == [0, 2, 3, 5, 6]
    assert meta[:5, 0].tolist() == [0, 2, 3, 5, 6] and meta[:5, 1].tolist() == [1, 2, 4, 1, 1] and counts.tolist() == [5, 0, 5]
    # nothing asked for, nothing taken: all padding
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(3, 8)
    assert CM.select(f, c, d, ep, 0, 3, 8, sel_slot, sel_dst, meta, pose, counts) == []
    assert sel_slot.tolist() == sel_dst.tolist() == [-1] * 3 and counts.tolist() == [0, 0, 0] and (meta == -7).all()


def test_overflow_of_per_turn_and_capacity_and_a_second_call():
    f, c, d = state([(1, 0, 0, 1, 3 + e, 3) for e in range(9)])
    ep = np.arange(20, 29, dtype=np.int32)
    # per_turn alone: 9 matches, 4 entries
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(4, 100)
    CM.select(f, c, d, ep, CM.ALL, 4, 100, sel_slot, sel_dst, meta, pose, counts)
    assert sel_slot.tolist() == [0, 1, 2, 3] and sel_dst.tolist() == [0, 1, 2, 3] and counts.tolist() == [4, 5, 9]
    # ... and a second call goes on behind the first: the same slots (nothing was rebuilt), the next rows
    CM.select(f, c, d, ep, CM.ALL, 4, 100, sel_slot, sel_dst, meta, pose, counts)
    assert sel_dst.tolist() == [4, 5, 6, 7] and meta[:8, 0].tolist() == [20, 21, 22, 23] * 2 and counts.tolist() == [8, 10, 18]
    assert (meta[8:] == -7).all()
    # capacity alone: room for 3 more of 9
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(16, 5, taken=2)
    CM.select(f, c, d, ep, CM.ALL, 16, 5, sel_slot, sel_dst, meta, pose, counts)
    assert sel_slot.tolist() == [0, 1, 2] + [-1] * 13 and sel_dst.tolist() == [2, 3, 4] + [-1] * 13 and counts.tolist() == [5, 6, 9]
    assert (meta[:2] == -7).all() and meta[2:, 3].tolist() == [0, 1, 2]
    # a full gallery takes nothing and counts on
    CM.select(f, c, d, ep, CM.ALL, 16, 5, sel_slot, sel_dst, meta, pose, counts)
    assert sel_slot.tolist() == [-1] * 16 and counts.tolist() == [5, 15, 18]
    # both together: per_turn 2 is the tighter, then the capacity
    sel_slot, sel_dst, meta, pose, counts = CM.fresh(2, 3)
    CM.select(f, c, d, ep, CM.ALL, 2, 3, sel_slot, sel_dst, meta, pose, counts)
    assert sel_dst.tolist() == [0, 1] and counts.tolist() == [2, 7, 9]
    CM.select(f, c, d, ep, CM.ALL, 2, 3, sel_slot, sel_dst, meta, pose, counts)
    assert sel_slot.tolist() == [0, -1] and sel_dst.tolist() == [2, -1] and counts.tolist() == [3, 15, 18]


# ---------------------------------------------------------------------------------------------------------------- the ABI
class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def test_the_header_against_the_binder():
    kinds = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32}
    declared = dict(re.findall(r'^int\s*(d2d_\w+)\(([^;]*)\);', HEADER, re.M))
    assert sorted(declared) == sorted('d2d_' + n for n in A.CAPTURE_ENTRY_POINTS) == ['d2d_capture_select', 'd2d_render_frame_sel',
                                                                                    'd2d_render_list_sel']
    bound = A.bind_capture(Recorder())
    for name, args in declared.items():
        want = []
        for a in args.replace('\n', ' ').strip().split(','):
            words = a.replace('*', ' * ').split()
            want.append((C.POINTER(A.Cfg) if 'd2d_cfg' in words else C.POINTER(A.State) if 'd2d_state' in words else
                         C.POINTER(A.RenderCall) if 'd2d_render_call' in words else C.c_void_p) if '*' in words
                        else kinds[[w for w in words if w != 'const'][0]])
        assert bound[name[len('d2d_'):]].argtypes == want and bound[name[len('d2d_'):]].restype is C.c_int, name
    define = lambda n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', HEADER).group(1), 0)          # noqa: E731
    assert define('D2D_RENDER_SKIPPED') == A.RENDER_SKIPPED == 3 and define('D2D_CAPTURE_META_F') == A.CAPTURE_META_F == 4
    assert define('D2D_CAPTURE_KINDS') == A.CAPTURE_KINDS == 6 and define('D2D_CAPTURE_COUNTS') == A.CAPTURE_COUNTS == 3
    assert [define('D2D_CAPTURE_' + n.upper()) for n in A.CAPTURE_KIND_NAMES] == [1, 2, 3, 4, 5, 6]
    assert [define('D2D_CAPTURE_M_' + n) for n in ('EPISODE', 'KIND', 'STEPS', 'SLOT')] == [0, 1, 2, 3]
    assert 'D2D_RENDER_VERSION' not in re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S) and A.D2D_RENDER_VERSION == 1
    assert not set(bound) & set(A.bind_render(Recorder()))


@pytest.mark.parametrize('missing', A.CAPTURE_ENTRY_POINTS)
def test_a_library_without_a_symbol_announces_no_capture(missing):
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_' + missing:
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    hb = _lib.HipBackend.__new__(_lib.HipBackend)
    hb.vfn = dict(A.bind_render(Old()), **A.bind_capture(Old()))
    assert hb.supports_capture is False and missing not in hb.vfn
    hb.vfn = dict(A.bind_render(Recorder()), **A.bind_capture(Recorder()))
    assert hb.supports_capture is True
    assert all(callable(getattr(_lib.HipBackend, n)) for n in A.CAPTURE_ENTRY_POINTS)


def test_the_built_library_exports_them_and_refuses_bad_arguments_without_a_gpu():
    lib, fn = _lib.load_render_library()
    fn = A.bind_capture(lib)
    assert sorted(fn) == sorted(A.CAPTURE_ENTRY_POINTS)
    err = lambda: A.bind_render(lib)['last_error']().decode()         # noqa: E731
    cfg, st, call = A.Cfg(), A.State(), A.RenderCall()
    assert fn['capture_select'](None, None, None, 3, 4, 8, None, None, None, None, None, None) == -1 and 'NULL' in err()
    assert fn['capture_select'](C.byref(cfg), C.byref(st), None, 3, 4, 8, None, None, None, None, None, None) == -2
    cfg.abi_version = A.D2D_ABI_VERSION
    assert fn['capture_select'](C.byref(cfg), C.byref(st), None, 1 << 6, 4, 8, None, None, None, None, None, None) == -1 and 'kinds' in err()
    assert fn['capture_select'](C.byref(cfg), C.byref(st), None, 3, -1, 8, None, None, None, None, None, None) == -1
    assert fn['capture_select'](C.byref(cfg), C.byref(st), None, 3, 4, 8, None, None, None, None, None, None) == -1 and 'counts' in err()
    assert fn['render_list_sel'](None, None, None, None) == -1 and 'd2d_render_list_sel' in err()
    assert fn['render_frame_sel'](C.byref(cfg), C.byref(st), C.byref(call), None, -1, None) == -1


# ---------------------------------------------------------------------------------------------------------------- the PNG encoder
def decode(png):
    """the [H, W, 3] array of an 8-bit RGB PNG whose rows all have filter 0"""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(png):
        n, tag = struct.unpack('>I4s', png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize('shape', [(130, 200), (7, 5), (1, 1), (3, 67)])
def test_png_round_trip(shape):
    rs = np.random.RandomState(shape[1])
    a = rs.randint(0, 256, size=shape + (3,)).astype(np.uint8)
    assert np.array_equal(decode(capture.png_bytes(a)), a)
    assert np.array_equal(decode(capture.png_bytes(a[:, ::-1])), a[:, ::-1])       # a view that is not contiguous
    with pytest.raises(ValueError):
        capture.png_bytes(a[..., :2])


def test_file_names():
    assert capture.file_name('LookAhead', 1, 73412) == 'LookAhead_static_000073412.png'
    assert capture.file_name('Owl', 2, 0) == 'Owl_dynamic_000000000.png' and capture.file_name('x', 6, A.STREAM_MAX_EPISODES) == 'x_other_268435455.png'
    assert [capture.file_name('g', k, 5).split('_', 1)[1][:-14] for k in range(1, 7)] == list(CM.NAMES)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(pkg):
    import tracks_backend as TB
    p = pkg.Params(**SMALL)
    plain = TB.env_of(p, 3)
    with pytest.raises(NotImplementedError, match='has no capture'):
        capture.Capture(plain)
    plain.backend = type('NoRenderer', (type(plain.backend),), {'supports_capture': True})()
    with pytest.raises(NotImplementedError, match='has no renderer'):
        capture.Capture(plain)
    env = CB.env_of(p, 3)
    with pytest.raises(ValueError, match="kind 'crash'"):
        capture.Capture(env, kinds=('static', 'crash'))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match='capacity'):
            capture.Capture(env, capacity=bad)
    for bad in (0, 4, 1.5):
        with pytest.raises(ValueError, match='per_turn'):
            capture.Capture(env, per_turn=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match='downsample'):
            capture.Capture(env, downsample=bad)
    cap = capture.Capture(env, kinds='goal', capacity=2, downsample=3)
    assert cap.per_turn == 3 and cap.kind_mask == 16 and tuple(cap.frames.shape) == (2, 44, 67, 3) and cap.frames.dtype == torch.uint8
    assert tuple(cap.meta.shape) == (2, 4) and cap.meta.dtype == torch.int32 and tuple(cap.pose.shape) == (2, 3) and cap.pose.dtype == torch.float64
    assert (cap.taken(), cap.dropped(), cap.matched()) == (0, 0, 0) and cap.save('/nonexistent/never/made') == []
    # the buffers are the capture's own: no holder of the env knows them, and the env's render scratch is not touched
    assert not any('capture' in n or 'render' in n for n, _, _ in env.fork_items()) and '_render' not in env.__dict__
    other = CB.env_of(p, 3)
    with pytest.raises(ValueError, match='another env'):
        other.action_stream(4, capture=cap)
    stream = env.action_stream(4, capture=cap)
    with pytest.raises(RuntimeError, match='still open'):
        cap.attach(env, object())
    with pytest.raises(RuntimeError, match='still open'):      # (what a second stream's constructor calls first)
        type(stream)(env, 4, 3, None, 1, None, cap)
    with pytest.raises(RuntimeError, match='open stream'):
        cap.snapshot()
    stream.close()
    cap.attach(env, stream)             # free again
    cap.detach(stream)
    # a stream whose constructor raises has not taken the capture
    fresh = CB.env_of(p, 3)
    cap2 = capture.Capture(fresh)
    fresh._stream_arrays = lambda *a, **k: (_ for _ in ()).throw(RuntimeError('no arrays'))
    with pytest.raises(RuntimeError, match='no arrays'):
        fresh.action_stream(4, capture=cap2)
    assert cap2._owner is None
    del fresh._stream_arrays
    fresh.action_stream(4, capture=cap2).close()
    assert cap2._owner is None


# ---------------------------------------------------------------------------------------------------------------- whole streams
def drive(stream, M):
    """Steps `stream` with a = policy(episode, steps) of the step a slot is about to play (the turn queued in front of the policy, as
    action_stream_cases.drive does) until every episode is handed out and none plays: the last ones are left for close() to harvest"""
    import action_stream_backend as AB
    _, _, done, info = stream.result()
    calls = 0
    while int(stream.counts[0]) < M or not bool(done[info['episode'] >= 0].all()):
        stream.turn()
        _, _, done, info = stream.step(AB.policy(info['episode'], info['steps']))
        calls += 1
        assert calls < 400
    return calls


def wide_frames(pkg, p, M, d=1):
    """(frames [M, Hf, Wf, 3], rows [M, 8], pose [M, 3]) of a batch of M envs of the same map ids played to the end"""
    from drone2d_amd import runner
    env = CB.env_of(p, M)
    stream = env.action_stream(M)
    drive(stream, M)
    frames = env.render_frames(downsample=d).numpy().copy()
    pose = env.state.drone[:, :3].numpy().copy()
    rows = runner.batch_records(env)
    stream.close()
    assert np.array_equal(stream.rows.numpy(), rows)
    return frames, rows, pose


def test_an_action_stream_s_gallery_is_the_terminal_pictures(pkg, tmp_path):
    """8 episodes through 3 slots under actions that depend on (episode, step) alone, every kind captured: frame, kind, steps and pose
    of every episode are those of a batch of 8 played to the end and rendered; the episodes only close() harvests are among them"""
    p, M = pkg.Params(**SMALL), 8
    want, rows, pose = wide_frames(pkg, p, M, 2)
    env = CB.env_of(p, 3)
    cap = capture.Capture(env, kinds=capture.ALL_KINDS, capacity=M, downsample=2)
    cap.frames.fill_(0xAB)
    stream = env.action_stream(M, refill_every=3, capture=cap)
    drive(stream, M)
    before = cap.taken()
    stream.close()
    assert before < M and cap.taken() == M == cap.matched() and cap.dropped() == 0
    assert np.array_equal(stream.rows.numpy(), rows)
    meta = cap.meta.numpy()
    assert sorted(meta[:, 0].tolist()) == list(range(M))
    for i in range(M):
        k = int(meta[i, 0])
        assert np.array_equal(cap.frames[i].numpy(), want[k]), k
        assert meta[i, 1] == CM.row_kind(rows[k]) and meta[i, 2] == rows[k, 0] and np.array_equal(cap.pose[i].numpy(), pose[k]), k
    assert len({w.tobytes() for w in want}) == M
    # the files: <gaze>_<kind>_<episode>.png, each the frame
    paths = cap.save(str(tmp_path / 'shots'))
    assert [os.path.basename(q) for q in paths] == [capture.file_name(p.gaze_method, meta[i, 1], meta[i, 0]) for i in range(M)]
    assert all(np.array_equal(decode(open(q, 'rb').read()), cap.frames[i].numpy()) for i, q in enumerate(paths))
    assert os.path.basename(cap.save(str(tmp_path), prefix='run7')[0]).startswith('run7_')


def episode_stream(pkg, p, M, B, **kw):
    from drone2d_amd import runner
    backend = CB.backend_for(p)
    xs = runner.EpisodeStream(p, M, B, device='cpu', backend=backend, **kw)
    backend.attach(xs.env)
    return xs


def test_record_img_is_the_reference_s_condition(pkg, tmp_path):
    """params.record_img with a gaze method other than NoControl: the static and dynamic collisions of the stream are saved into
    params.img_dir under the reference's names; NoControl, or no record_img, builds no capture and writes nothing"""
    cell = dict(SMALL, gaze_method='LookAhead', agent_number=10, agent_radius=10)
    for kw in (dict(record_img=False), dict(record_img=True, gaze_method='NoControl')):
        xs = episode_stream(pkg, pkg.Params(**dict(cell, img_dir=str(tmp_path / 'none'), **kw)), 2, 2)
        assert xs.capture is None
        xs.run(refill_every=8)
        assert xs.image_paths == [] and not (tmp_path / 'none').exists()
    p = pkg.Params(**dict(cell, record_img=True, img_dir=str(tmp_path / 'img')))
    xs = episode_stream(pkg, p, 8, 3)
    assert isinstance(xs.capture, capture.Capture) and xs.capture.kinds == ('static', 'dynamic') and xs.capture.per_turn == 3
    rows = xs.run(refill_every=5)
    crashed = {k: ('static' if r[17] else 'dynamic') for k, r in enumerate(rows) if r[17] or r[18]}
    assert len(crashed) >= 1, rows
    assert sorted(os.listdir(p.img_dir)) == sorted(f'LookAhead_{kind}_{k:09d}.png' for k, kind in crashed.items())
    assert sorted(xs.image_paths) == sorted(os.path.join(p.img_dir, n) for n in os.listdir(p.img_dir))
    assert xs.capture.matched() == len(crashed) == xs.capture.taken() and xs.capture._owner is None
    assert decode(open(xs.image_paths[0], 'rb').read()).shape == (130, 200, 3)
    # a capture of the caller's making, built on the stream's env; nothing is saved without record_img
    q = pkg.Params(**dict(cell, img_dir=str(tmp_path / 'mine')))
    xs = episode_stream(pkg, q, 4, 2, capture=lambda env: capture.Capture(env, capture.ALL_KINDS, capacity=4, downsample=4))
    xs.run(refill_every=7)
    assert xs.capture.taken() == 4 and xs.image_paths == [] and not (tmp_path / 'mine').exists()
    assert sorted(xs.capture.meta[:, 0].tolist()) == [0, 1, 2, 3] and xs.capture.meta[:, 2].tolist() == [int(xs.records[k, 0]) for k in xs.capture.meta[:, 0].tolist()]
    # ... nor with record_img under NoControl, which is outside the reference's condition
    q = pkg.Params(**dict(cell, record_img=True, gaze_method='NoControl', img_dir=str(tmp_path / 'mine')))
    xs = episode_stream(pkg, q, 3, 2, capture=lambda env: capture.Capture(env, capture.ALL_KINDS, capacity=3, downsample=4))
    xs.run(refill_every=7)
    assert xs.capture.taken() == 3 and xs.image_paths == [] and not (tmp_path / 'mine').exists()
