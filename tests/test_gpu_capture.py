"""capture.Capture on the device (include/d2d_capture.h): d2d_capture_select against the model of tests/capture_model.py over hand-made
states inside poisoned buffers, the two skipping launches against render_frames() byte for byte, and whole streams -- the gallery of a
narrow stream against a wide env of the same episodes played to the end and rendered, for stream_episodes() and action_stream(), the
kind filter, both overflows, and snapshot().  Every comparison is exact.

Geometry: the renderer tests' small map, 200 x 130 px (2 x 5 tiles of 128 x 32 pixels with ragged edges), 4 agents, 2 pillars, a view
depth of 40, and a flight time of 3.5 s, so every episode ends within 36 steps."""
import functools

import numpy as np
import pytest
import torch

import action_stream_backend as AB
import capture_model as CM
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu

POISON = 0xAB
GUARD = 4096
SMALL = dict(planner='Primitive', gaze_method='Oxford', map_size=[200, 130], init_pos=[20, 20], target_list=[[180, 110]], agent_number=4,
             agent_radius=5, agent_max_speed=20, drone_max_speed=30, pillar_number=2, drone_view_depth=40, drone_view_range=120,
             max_flight_time=3.5, map_id=3)
M, SLOTS = 24, 8


def _env(hip, p, B, **kw):
    from drone2d_amd import vec_env
    kw.setdefault('gaze', 'external')
    kw.setdefault('worlds', 'device')
    return vec_env.VecDrone2DEnv(p, B, backend=hip, planner=p.planner, device_plugins=True, **kw)


def _guarded(nbytes, device):
    big = torch.full((GUARD * 2 + nbytes,), POISON, dtype=torch.uint8, device=device)
    return big, big[GUARD:GUARD + nbytes]


def _intact(big, nbytes):
    return bool((big[:GUARD] == POISON).all()) and bool((big[GUARD + nbytes:] == POISON).all())


def _state_bytes(env):
    return [(n, t.clone()) for n, t, _ in env.fork_items()]


def _unchanged(env, before):
    now = {n: t for n, t, _ in env.fork_items()}
    return [n for n, t in before if not torch.equal(t.reshape(-1).view(torch.uint8), now[n].reshape(-1).view(torch.uint8))]


# ---------------------------------------------------------------------------------------------------------------- 1. the selection
def test_select_is_the_model(pkg, hip):
    """B = 130 slots (three passes of 64, the last ragged) with flags and counters written by hand -- every kind, slots that are not
    done, slots without a step, retired slots -- through d2d_capture_select under seven argument sets, two calls each on the same
    buffers: every output equals the model's, the bytes around every buffer and the env's own tensors stay as they were"""
    assert hip.supports_capture
    B, dev = 130, hip.device
    env = _env(hip, pkg.Params(**SMALL), B)
    rs = np.random.RandomState(11)
    flags = np.stack([rs.choice([0, 0, 1, 2, 3], B), rs.rand(B) < 0.2, rs.rand(B) < 0.3, rs.rand(B) < 0.7], axis=1).astype(np.uint8)
    counters = env.state.counters.cpu().numpy().copy()
    counters[:, A.C_STEPS] = rs.choice([0, 1, 2, 17, 36], B)
    counters[:, A.C_SM] = rs.randint(0, 4, B)
    episode = np.where(rs.rand(B) < 0.2, -1, 1000 + rs.permutation(B)).astype(np.int32)
    env.state.flags.copy_(torch.from_numpy(flags))
    env.state.counters.copy_(torch.from_numpy(counters))
    env.state.drone[:, :3] = torch.from_numpy(rs.uniform(-5, 205, (B, 3))).to(dev)
    drone = env.state.drone.cpu().numpy()
    ep_dev = torch.from_numpy(episode).to(dev)
    kinds_seen = {CM.kind_of(flags[e], counters[e]) for e in range(B) if flags[e, 3]}
    assert kinds_seen == {1, 2, 3, 4, 5, 6} and (episode[128:] >= 0).any() and flags[64:128, 3].any()
    before = _state_bytes(env)
    cases = [(CM.ALL, 130, 200, 0, True), (CM.mask('static', 'dynamic'), 16, 200, 3, True), (CM.ALL, 130, 10, 4, True),
             (CM.ALL, 7, 9, 5, True), (CM.mask('freezing', 'other'), 64, 64, 0, False), (0, 5, 5, 0, True), (CM.mask('goal'), 1, 1, 0, False)]
    for kinds, S, capacity, taken, with_episode in cases:
        sizes = dict(sel_slot=4 * S, sel_dst=4 * S, meta=16 * capacity, pose=24 * capacity, counts=24)
        big, view = {}, {}
        for name, n in sizes.items():
            big[name], view[name] = _guarded(n, dev)
        sel_slot, sel_dst = view['sel_slot'].view(torch.int32), view['sel_dst'].view(torch.int32)
        meta, pose = view['meta'].view(torch.int32).view(capacity, 4), view['pose'].view(torch.float64).view(capacity, 3)
        counts = view['counts'].view(torch.int64)
        counts.copy_(torch.tensor([taken, 2, 40]))
        want = [t.cpu().numpy().copy() for t in (sel_slot, sel_dst, meta, pose, counts)]
        accepted = 0
        for call in range(2):
            hip.capture_select(env.cfg, env._st, ep_dev if with_episode else None, kinds, sel_slot, sel_dst, meta, pose, counts)
            hip.sync()
            accepted += len(CM.select(flags, counters, drone, episode if with_episode else None, kinds, S, capacity, *want))
            got = [t.cpu().numpy() for t in (sel_slot, sel_dst, meta, pose, counts)]
            for name, g, w in zip(('sel_slot', 'sel_dst', 'meta', 'pose', 'counts'), got, want):
                assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (kinds, S, capacity, call, name, g.tolist()[:8], w.tolist()[:8])
        assert all(_intact(big[n], sizes[n]) for n in sizes), (kinds, S, capacity)
        assert int(counts[0]) == taken + accepted <= max(capacity, taken) and int(counts[0] - taken + counts[1] - 2) == int(counts[2] - 40)
    assert _unchanged(env, before) == []


# ---------------------------------------------------------------------------------------------------------------- 2. skipped entries
@pytest.mark.parametrize('d', [1, 3])
def test_skipped_entries_write_nothing(pkg, hip, d):
    """eight entries over four slots 12 steps in: two name no slot (-1), two a frame outside the gallery, one a slot outside the
    batch, slot 2 is painted twice.  Poisoned beforehand: the lists, boxes and counts of the skipped entries and the frames nobody
    names keep the poison; each painted frame is render_frames() of its slot, byte for byte"""
    from drone2d_amd import render
    env = _env(hip, pkg.Params(**SMALL), 4)
    rs = np.random.RandomState(17)
    for t in range(12):
        env._set_action(torch.from_numpy(rs.uniform(-1, 1, 4)).to(env.device))
        env._plugins_step()
    dev, capacity = env.device, 6
    slots = torch.tensor([2, -1, 0, 2, -1, 3, 2, 99], dtype=torch.int32, device=dev)
    dst = torch.tensor([4, 1, 0, 9, 2, -3, 5, 3], dtype=torch.int32, device=dev)
    S = 8
    want = env.render_frames(downsample=d).cpu().numpy()
    before = _state_bytes(env)
    sc = render.RenderScratch()
    c, keep = render.call_of(env, slots, d, scratch=sc)
    for t in (sc.items, sc.bbox, sc.count, sc.status):
        t.view(torch.uint8).fill_(POISON)
    Hf, Wf = render.frame_shape(env.cfg, d)
    fbig, fview = _guarded(capacity * Hf * Wf * 3, dev)
    frames = fview.view(capacity, Hf, Wf, 3)
    c.frame = frames.data_ptr()
    hip.render_list_sel(env.cfg, env._st, c)
    hip.render_frame_sel(env.cfg, env._st, c, dst, capacity)
    hip.sync()
    assert sc.status.tolist() == [A.RENDER_OK, A.RENDER_SKIPPED, A.RENDER_OK, A.RENDER_OK, A.RENDER_SKIPPED, A.RENDER_OK, A.RENDER_OK,
                                  A.RENDER_BAD_SLOT]
    counts = sc.count.tolist()
    assert counts[1] == counts[4] == counts[7] == 0 and counts[0] == counts[3] == counts[6] > 0 and min(counts[2], counts[5]) > 0
    for k in (1, 4):
        assert bool((sc.items[k] == POISON).all()) and bool((sc.bbox[k].view(torch.uint8) == POISON).all()), k
    got = frames.cpu().numpy()
    assert np.array_equal(got[4], want[2]) and np.array_equal(got[5], want[2]) and np.array_equal(got[0], want[0])
    assert (got[3] == 240).all()                               # the slot outside the batch: UNEXPLORED, as d2d_render_frame leaves it
    assert (got[1] == POISON).all() and (got[2] == POISON).all() and _intact(fbig, capacity * Hf * Wf * 3)
    assert len({want[e].tobytes() for e in range(4)}) == 4
    # the same entries through the plain launches draw every entry: the skipping is the _sel launches' own
    plain = torch.full((S, Hf, Wf, 3), POISON, dtype=torch.uint8, device=dev)
    c.frame = plain.data_ptr()
    hip.render_list(env.cfg, env._st, c)
    hip.render_frame(env.cfg, env._st, c)
    hip.sync()
    assert sc.status.tolist() == [0, 2, 0, 0, 2, 0, 0, 2] and not bool((plain == POISON).all(dim=3).all(dim=2).all(dim=1).any())
    assert np.array_equal(plain[3].cpu().numpy(), want[2]) and _unchanged(env, before) == []


# ---------------------------------------------------------------------------------------------------------------- 3. stream_episodes
def _params(pkg, profile):
    return pkg.Params(**dict(SMALL, **({'motion_profile': 'RVO'} if profile == 'RVO' else {})))


@functools.lru_cache(maxsize=None)
def _wide_episodes(hip, profile):
    """(frames [M, 130, 200, 3] at downsample 1, records [M, 8], poses [M, 3], the env) of M envs of the stream's map ids under the
    device's Oxford gaze, played to the end by run_episodes() -- a finished env stays as it ended -- and rendered.  Computed once"""
    import drone2d_amd as pkg
    from drone2d_amd import runner
    p = _params(pkg, profile)
    env = _env(hip, p, M, gaze=p.gaze_method)
    env.run_episodes()
    assert bool(env.state.flags[:, A.F_DONE].all())
    frames = env.render_frames().cpu().numpy()
    return frames, runner.batch_records(env), env.state.drone[:, :3].cpu().numpy().copy(), env


def _assert_gallery(cap, n, frames, rows, pose, d):
    """gallery rows [0, n) against the wide env's: returns the episodes in gallery order"""
    meta, got, gpose = cap.meta[:n].cpu().numpy(), cap.frames[:n].cpu().numpy(), cap.pose[:n].cpu().numpy()
    for i in range(n):
        k = int(meta[i, A.CAPTURE_M_EPISODE])
        want = frames[k][::d, ::d]
        assert np.array_equal(got[i], want), (i, k, np.argwhere(got[i] != want)[:5].tolist())
        assert meta[i, A.CAPTURE_M_KIND] == CM.row_kind(rows[k]) and meta[i, A.CAPTURE_M_STEPS] == rows[k, A.STREAM_R_STEPS], (i, k)
        assert np.array_equal(gpose[i].view(np.uint64), pose[k].view(np.uint64)), (i, k)
    return meta[:, A.CAPTURE_M_EPISODE].tolist()


@pytest.mark.parametrize('profile,refill_every,d', [('CVM', 4, 1), ('CVM', 9, 1), ('CVM', 4, 3), ('CVM', 9, 3), ('RVO', 5, 1)])
def test_the_gallery_of_stream_episodes_is_the_terminal_pictures(pkg, hip, profile, refill_every, d):
    """24 episodes through 8 slots with every kind captured and room for all: for every k the gallery frame whose meta says episode k
    is frame k of the wide env, and its kind, steps and pose are those of rows[k] and of the wide env's state"""
    from drone2d_amd import capture
    frames, rows, pose, _ = _wide_episodes(hip, profile)
    p = _params(pkg, profile)
    env = _env(hip, p, SLOTS, gaze=p.gaze_method)
    cap = capture.Capture(env, kinds=capture.ALL_KINDS, capacity=M, downsample=d)
    assert cap.per_turn == SLOTS
    got_rows = env.stream_episodes(M, refill_every=refill_every, capture=cap).cpu().numpy()
    assert np.array_equal(got_rows, rows) and (rows[:, A.STREAM_R_STEPS] > 0).all()
    assert (cap.taken(), cap.dropped(), cap.matched()) == (M, 0, M) and cap._owner is None
    order = _assert_gallery(cap, M, frames, rows, pose, d)
    assert sorted(order) == list(range(M)) and order != list(range(M))          # arrival order: the schedule's, not the episodes'
    assert len({f.tobytes() for f in frames}) == M and len(set(rows[:, A.STREAM_R_STEPS].tolist())) > 1


# ---------------------------------------------------------------------------------------------------------------- 4. action_stream
def _drive(stream, m):
    """a = policy(episode, steps) of the step a slot is about to play, the turn queued in front of the policy (as
    action_stream_cases.drive does); stops when every episode is handed out and none plays, so the last are left to close()"""
    _, _, done, info = stream.result()
    calls = 0
    while int(stream.counts[0]) < m or not bool(done[info['episode'] >= 0].all()):
        stream.turn()
        _, _, done, info = stream.step(AB.policy(info['episode'], info['steps']))
        calls += 1
        assert calls < 600
    return calls


@pytest.mark.parametrize('planner', ['Primitive', 'Jerk_Primitive'])
def test_the_gallery_of_an_action_stream_is_the_terminal_pictures(pkg, hip, planner):
    """the same for a stream the caller steps: 24 episodes through 8 slots against a wide stream of 24 slots that is never refilled,
    rendered before its close(); the episodes that only close() harvests are in the gallery"""
    from drone2d_amd import capture, runner
    p = pkg.Params(**dict(SMALL, planner=planner))
    wide = _env(hip, p, M)
    ws = wide.action_stream(M)
    _drive(ws, M)
    frames, rows, pose = wide.render_frames().cpu().numpy(), runner.batch_records(wide), wide.state.drone[:, :3].cpu().numpy().copy()
    ws.close()
    assert np.array_equal(ws.rows.cpu().numpy(), rows)
    env = _env(hip, p, SLOTS)
    cap = capture.Capture(env, kinds=capture.ALL_KINDS, capacity=M + 3, downsample=2)
    cap.frames.fill_(POISON)
    stream = env.action_stream(M, refill_every=3, capture=cap)
    _drive(stream, M)
    early = cap.taken()
    stream.close()
    assert 0 < early < M and (cap.taken(), cap.dropped(), cap.matched()) == (M, 0, M) and cap._owner is None
    assert np.array_equal(stream.rows.cpu().numpy(), rows)
    order = _assert_gallery(cap, M, frames, rows, pose, 2)
    assert sorted(order) == list(range(M)) and bool((cap.frames[M:] == POISON).all()) and bool((cap.meta[M:] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- 5. filter, overflow
def test_the_kind_filter_and_both_overflows(pkg, hip):
    """kinds=('freezing',): the captured episodes are exactly the rows that say freezing.  Map ids 3 .. 26 of the small CVM cell under
    Oxford's gaze: on the CPU oracle's closed loop 16 episodes end by freezing (the flight time runs out), 5 by a dynamic and 3 by a
    static collision, so 0 < matched = 16 < 24.  Then capacity 5 and per_turn 2 with every kind: five frames, the rest counted as dropped; the
    gallery, meta and pose sit inside larger poisoned buffers, and every byte from row 5 on keeps its poison"""
    from drone2d_amd import capture
    frames, rows, pose, _ = _wide_episodes(hip, 'CVM')
    p = _params(pkg, 'CVM')
    freezing = [k for k in range(M) if CM.row_kind(rows[k]) == CM.FREEZING]
    print('kinds of the', M, 'episodes:', [CM.NAMES[CM.row_kind(r) - 1] for r in rows])
    env = _env(hip, p, SLOTS, gaze=p.gaze_method)
    cap = capture.Capture(env, kinds=('freezing',), capacity=M)
    cap.frames.fill_(POISON)
    env.stream_episodes(M, refill_every=6, capture=cap)
    n = cap.taken()
    assert 0 < cap.matched() < M and n == cap.matched() == len(freezing) and cap.dropped() == 0
    assert sorted(_assert_gallery(cap, n, frames, rows, pose, 1)) == freezing and bool((cap.frames[n:] == POISON).all())
    env = _env(hip, p, SLOTS, gaze=p.gaze_method)
    cap = capture.Capture(env, kinds=capture.ALL_KINDS, capacity=5, per_turn=2, downsample=2)
    # the gallery, meta and pose each lie inside a larger poisoned buffer with room for three more rows behind them and a guard band
    # on either side: a frame 5, 6 or 7, or a row of meta or pose beyond the capacity, would land in bytes that are checked below
    Hf, Wf = cap.frames.shape[1:3]
    used = dict(frames=5 * Hf * Wf * 3, meta=5 * 16, pose=5 * 24)
    big = {n: torch.full((GUARD + u // 5 * 8 + GUARD,), POISON, dtype=torch.uint8, device=env.device) for n, u in used.items()}
    cap.frames = big['frames'][GUARD:GUARD + used['frames']].view(5, Hf, Wf, 3)
    cap.meta = big['meta'][GUARD:GUARD + used['meta']].view(torch.int32).view(5, 4)
    cap.pose = big['pose'][GUARD:GUARD + used['pose']].view(torch.float64).view(5, 3)
    env.stream_episodes(M, refill_every=6, capture=cap)
    assert cap.taken() == 5 and cap.matched() == M and cap.taken() + cap.dropped() == cap.matched()
    order = _assert_gallery(cap, 5, frames, rows, pose, 2)
    assert len(set(order)) == 5
    for n, u in used.items():                  # frames 5 and beyond, rows 5 and beyond, and both guard bands keep their poison
        assert bool((big[n][:GUARD] == POISON).all()) and bool((big[n][GUARD + u:] == POISON).all()), n
        assert not bool((big[n][GUARD:GUARD + u] == POISON).all()), n          # (the launches did write into these buffers)


# ---------------------------------------------------------------------------------------------------------------- 6. snapshot
def test_snapshot_of_a_batch_is_render_frames_of_its_done_slots(pkg, hip):
    """the wide env after run_episodes(): snapshot() with two kinds takes every done slot of those kinds in slot order, episode =
    slot, whatever per_turn says; a second call takes them again; nothing of the env is written"""
    from drone2d_amd import capture
    frames, rows, pose, env = _wide_episodes(hip, 'CVM')
    kinds = ('static', 'freezing', 'goal')
    want = [k for k in range(M) if CM.NAMES[CM.row_kind(rows[k]) - 1] in kinds]
    assert 2 < len(want)
    before = _state_bytes(env)
    cap = capture.Capture(env, kinds=kinds, capacity=2 * len(want) + 1, per_turn=2)
    cap.frames.fill_(POISON)
    assert cap.snapshot() is cap and cap.taken() == len(want) == cap.matched()
    assert _assert_gallery(cap, len(want), frames, rows, pose, 1) == want and cap.meta[:len(want), A.CAPTURE_M_SLOT].tolist() == want
    cap.snapshot()
    assert cap.taken() == 2 * len(want) and cap.meta[len(want):2 * len(want), 0].tolist() == want and cap.dropped() == 0
    assert bool((cap.frames[2 * len(want):] == POISON).all()) and _unchanged(env, before) == [] and '_render' in env.__dict__
    assert env._render.key[0] == M              # the env's own scratch is the one render_frames() left, not the capture's
