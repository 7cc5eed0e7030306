"""swept_obs=True on the device (include/d2d_swept.h: d2d_swept_mark, d2d_swept_crop): the reference's recorded maps through the HIP
library step for step, handmade trajectories through the two launches alone over poisoned buffers, a random soak against the numpy
model of tests/swept_model.py evaluated on a snapshot taken between the mark and the plan launch, a stream with the channel (one
launch per stage) against the same stream without it (the persistent kernel), and Jerk_Primitive's zeros.  Every comparison is exact
equality of integers."""
import numpy as np
import pytest
import torch

import action_stream_cases as AC
import swept_cases as SC
import swept_model as SW
from action_stream_backend import policy
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu


def _env(hip, p, B, **kw):
    from drone2d_amd import vec_env
    kw.setdefault('gaze', 'external')
    return vec_env.VecDrone2DEnv(p, B, backend=hip, planner=p.planner, device_plugins=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('i', range(SC.EPISODES))
def test_the_recorded_episodes_through_the_library(pkg, hip, i):
    assert hip.supports_swept_obs
    trunc, empty, longest, lost = SC.coverage()
    assert trunc >= 5 and empty >= 5 and longest > 128 and lost >= 1, (trunc, empty, longest, lost)
    ep = SC.episode(i)
    env = _env(hip, SC.params_of(pkg, ep), 1, swept_obs=True)
    assert SC.replay(env, ep) == len(ep['action'])


# ---------------------------------------------------------------------------------------------------------------- 2. handmade
POISON = 0xAB


def _path(n, start, step=(2.0, 0.0)):
    i = np.arange(n, dtype=np.float64)
    return np.stack([start[0] + i * step[0], start[1] + i * step[1]], axis=1)


def _there_and_back(n, start):
    """2 px a waypoint along x for 35 waypoints, back for 35 -- waypoint 70 is waypoint 0's position again -- then along y"""
    i = np.arange(n)
    x = np.where(i <= 35, i, np.where(i <= 70, 70 - i, 0)) * 2.0 + start[0]
    y = np.where(i <= 70, 0, i - 70) * 2.0 + start[1]
    return np.stack([x, y], axis=1).astype(np.float64)


def _handmade_cases():
    """per env: head, the waypoints, the trackers (mx, my, vx, vy, active, prev, radius, lim), the drone's position, done, and m
    where the case is built for one (None: whatever the model says)"""
    on = lambda xy, lim=1e-6, act=1, prev=1, rad=10.0, v=(0.0, 0.0): (xy[0], xy[1], v[0], v[1], act, prev, rad, lim)   # noqa: E731
    cases = []
    add = lambda **kw: cases.append(dict(dict(head=0, trk=[], drone=(250.0, 250.0), done=0, m=None), **kw))   # noqa: E731
    centre, a = (250.0, 250.0), (20.0, 30.0)
    add(way=_path(0, a), m=0)                                                               # n = 0
    add(way=_path(1, a), m=1, drone=(0.0, 0.0))                                             # n = 1; the drone in a corner
    w = _path(63, (300.0, 30.0))
    add(way=w, trk=[on(w[62])], m=63, drone=(499.0, 0.0))                                   # a hit at n - 1
    w = _path(64, (20.0, 450.0))
    add(way=w, trk=[on(w[63])], m=64, drone=(0.0, 499.0))                                   # a hit at 63: the last lane of a pass
    w = _path(65, (330.0, 470.0))
    add(way=w, trk=[on(w[64])], m=65, drone=(499.0, 499.0))                                 # a hit at 64: the first lane of the next
    w = _there_and_back(200, (200.0, 200.0))
    add(way=w, m=200, drone=centre)                                                         # leaves a cell, re-enters it 70 later
    w = _path(130, (150.0, 250.0))
    add(head=70, way=w, trk=[on(w[0])], m=1, drone=centre)                                  # head = 70, stored = 200; a hit at i = 0
    add(head=70, way=w, m=130, drone=centre)                                                # ... and none: passes across the chunks
    w = _path(200, (60.0, 240.0))
    add(way=w, trk=[on(w[150]), on(w[100])], m=101, drone=centre)                           # two trackers, different i
    add(way=w, trk=[on(w[40], act=0, prev=1), on(w[90], act=0, prev=0)], m=200, drone=centre)   # inactive trackers on the path
    # a tracker that crosses the path at waypoint 20; trk_lim == 0: the radius decides ... and the same limit, cached ('radius')
    add(way=w, trk=[on((100.0, 300.0), lim=0.0, rad=12.0, v=(0.0, -30.0))], drone=centre)
    add(way=w, trk=[on((100.0, 300.0), lim='radius', rad=12.0, v=(0.0, -30.0))], drone=centre)
    w = _path(200, (-21.0, 250.0), step=(2.75, 0.0))
    add(way=w, m=200, drone=(20.0, 250.0))                                                  # waypoints outside the map: x < 0, x >= 500
    w = _path(200, a)
    add(way=w, trk=[on(w[0])], m=1, drone=a)                                                # a hit at i = 0
    add(way=w, trk=[on(w[128])], m=129, drone=a, done=1)                                    # a done env: nothing is written
    add(way=_there_and_back(200, (400.0, 20.0)), trk=[on((400.0, 160.0), lim=0.0, rad=5.0)], drone=(420.0, 40.0))
    assert len(cases) == 16
    return cases


def test_handmade_trajectories_through_the_two_launches_alone(pkg, hip):
    cases = _handmade_cases()
    B = len(cases)
    p = pkg.Params(planner='Primitive', agent_number=3, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=0)
    env = _env(hip, p, B, swept_obs=True)
    cfg, N, cap = env.cfg, env.cfg.N, env.plugins.t['traj'].shape[1]
    assert (cfg.W, cfg.H, N) == (50, 50, 3) and cap >= 200
    traj, hdr = np.zeros((B, cap, 4)), np.zeros((B, 2), dtype=np.int32)
    kf = env.state.kf.cpu().numpy().copy()
    active, prev = np.zeros((B, N), dtype=np.uint8), np.zeros((B, N), dtype=np.uint8)
    rad, lim = np.full((B, N), 10.0), np.zeros((B, N))
    drone, flags = env.state.drone.cpu().numpy().copy(), np.zeros((B, 4), dtype=np.uint8)
    rs = np.random.RandomState(5)
    traj[:, :, :2] = rs.uniform(0, 500, size=(B, cap, 2))          # whatever lies outside [head, stored) must not matter
    for e, c in enumerate(cases):
        n = len(c['way'])
        traj[e, c['head']:c['head'] + n, :2] = c['way']
        hdr[e] = c['head'], c['head'] + n
        for k, t in enumerate(c['trk']):
            kf[e, k, :4] = t[:4]
            active[e, k], prev[e, k], rad[e, k] = t[4:7]
            lim[e, k] = SW.sq_threshold(float(cfg.drone_radius) + t[6]) if t[7] == 'radius' else t[7]
        drone[e, A.D_X], drone[e, A.D_Y] = c['drone']
        flags[e, A.F_DONE] = c['done']
    dev = env.device
    pt, st = env.plugins.t, env.state
    for t, v in ((pt['traj'], traj), (pt['traj_hdr'], hdr), (st.kf, kf), (st.active, active), (pt['trk_prev'], prev), (pt['trk_radius'], rad),
                 (pt['trk_lim'], lim), (st.drone, drone), (st.flags, flags)):
        t.copy_(torch.from_numpy(v).to(dev))
    for name in ('map', 'obs', 'count'):
        env.swept[name].view(torch.uint8).fill_(POISON)
    env.swept['live'].fill_(7)
    keep = {k: pt[k].clone() for k in ('traj', 'traj_hdr', 'trk_radius', 'trk_prev', 'trk_lim')}
    hip.swept_mark(cfg, env._st, env._plan, env._swept)
    hip.swept_crop(cfg, env._st, env._swept)
    hip.sync()
    for k, v in keep.items():                                      # the mark only reads the plugin state
        assert torch.equal(pt[k].view(torch.uint8), v.view(torch.uint8)), k
    full, crop, count, live = (env.swept[k].cpu().numpy() for k in ('map', 'obs', 'count', 'live'))
    poison32 = int(np.full(4, POISON, dtype=np.uint8).view(np.int32)[0])
    reentered = 0
    for e, c in enumerate(cases):
        if c['done']:
            assert live[e] == 0 and (full[e] == POISON).all() and (crop[e] == POISON).all() and count[e] == poison32, e
            continue
        want, m = SW.mark(traj[e], hdr[e, 0], hdr[e, 1], kf[e], active[e], rad[e], lim[e], cfg)
        assert c['m'] is None or m == c['m'], (e, m, c['m'])       # the case is what it was built to be
        assert live[e] == 1 and count[e] == m, (e, int(count[e]), m)
        assert np.array_equal(full[e], want), (e, np.argwhere(full[e] != want)[:5].tolist())
        assert np.array_equal(crop[e], SW.crop(want, c['drone'], cfg)), e
        if e in (5, 15):                                            # the re-entered cell holds the LATER waypoint's value (70 * dt = 7)
            w0 = c['way'][0]
            reentered += int(want[int(w0[0] // 10), int(w0[1] // 10)] == 7)
    assert reentered >= 1 and len({int(c) for c in count}) > 6
    m10 = int(count[10])
    assert 1 < m10 < 200 and m10 == int(count[11])                 # the cached limit and the one found from the radius agree
    assert m10 < 21 and lim[11, 0] > 0 and lim[10, 0] == 0
    assert full[12].any() and all(crop[e].any() for e in (2, 3, 4, 5, 12))       # every corner, the centre, the map's edge


# ---------------------------------------------------------------------------------------------------------------- 3. random soak
def test_random_soak_against_the_model(pkg, hip):
    """64 seeded worlds x 120 steps, 30 agents at speed 40 and radius 10, random actions.  The model runs on what the mark read: a
    snapshot taken between the mark and the plan launch (_plugins_step's hook).  Coverage, not tolerance: at least 10 truncated maps
    and a trajectory above 128 waypoints, or the test has not looked where the stage can go wrong"""
    B, T = 64, 120
    p = pkg.Params(planner='Primitive', agent_number=30, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=1000)
    env = _env(hip, p, B, swept_obs=True, worlds='device')
    pt, st, cfg, N = env.plugins.t, env.state, env.cfg, env.cfg.N
    gen = torch.Generator().manual_seed(11)
    snap = {}

    def snapshot():
        for k, t in (('traj', pt['traj']), ('hdr', pt['traj_hdr']), ('rad', pt['trk_radius']), ('lim', pt['trk_lim']), ('prev', pt['trk_prev']),
                     ('kf', st.kf), ('active', st.active), ('done', st.flags)):
            snap[k] = t.clone()

    truncated = longest = marked = frozen = 0
    last = None
    for t in range(T):
        env._set_action(torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1)
        env._plugins_step(before_plan=snapshot)
        h = {k: v.cpu().numpy() for k, v in snap.items()}
        full, crop, count, live = (env.swept[k].cpu().numpy() for k in ('map', 'obs', 'count', 'live'))
        drone = st.drone.cpu().numpy()
        for e in range(B):
            if h['done'][e, A.F_DONE]:                              # finished before the step: everything as it was
                assert live[e] == 0 and np.array_equal(full[e], last[0][e]) and np.array_equal(crop[e], last[1][e]) and count[e] == last[2][e]
                frozen += 1
                continue
            want, m = SW.mark(h['traj'][e], h['hdr'][e, 0], h['hdr'][e, 1], h['kf'][e], h['active'][e, :N], h['rad'][e, :N], h['lim'][e, :N], cfg)
            n = int(h['hdr'][e, 1] - h['hdr'][e, 0])
            assert live[e] == 1 and count[e] == m, (t, e, int(count[e]), m, n)
            assert np.array_equal(full[e], want), (t, e)
            assert np.array_equal(crop[e], SW.crop(want, drone[e, :2], cfg)), (t, e)
            truncated += int(m < n)
            longest = max(longest, n)
            marked += int(m > 0)
        last = (full, crop, count)
    assert truncated >= 10 and longest > 128, (truncated, longest)
    assert marked > B * T // 4 and frozen > 0, (marked, frozen)


# ---------------------------------------------------------------------------------------------------------------- 4. the stream
def test_a_stream_with_the_channel_equals_the_stream_without(pkg, hip):
    """8 slots, 24 episodes, a turn every 4 steps: swept_obs=True steps stage by stage, swept_obs=False through the persistent kernel"""
    slots, M = 8, 24
    p = AC.params_of(pkg, 'Primitive-CVM')
    a = _env(hip, p, slots, swept_obs=True, worlds='device').action_stream(M, refill_every=4)
    b = _env(hip, p, slots, worlds='device').action_stream(M, refill_every=4)
    info = a.result()[3]
    calls = marked = zero_at_0 = 0
    while a.finished_now() < M:
        assert calls < 2000
        last = info['episode'].clone()
        assert a.turn() == b.turn()
        obs, _, _, info = a.result()
        fresh = (info['episode'] != last) & (info['episode'] >= 0)
        if bool(fresh.any()):                                       # a refilled slot: a zero map at its step 0
            assert not bool(obs['swep_map'][fresh].any()) and not bool(a.env.swept_map[fresh].any())
            assert not bool(a.env.swept_count[fresh].any()) and not bool(info['steps'][fresh].any())
            zero_at_0 += int(fresh.sum())
        act = policy(info['episode'], info['steps'])
        oa, ta, da, ia = a.step(act)
        ob, tb, db, ib = b.step(act)
        assert torch.equal(a.rows, b.rows) and torch.equal(da, db), calls
        assert all(torch.equal(ta[k], tb[k]) for k in ta) and all(torch.equal(ia[k], ib[k]) for k in ia), calls
        assert torch.equal(oa['local_map'], ob['local_map']) and torch.equal(oa['yaw_angle'], ob['yaw_angle']), calls
        marked += int(oa['swep_map'].any())
        info = ia
        calls += 1
    a.close(), b.close()
    assert torch.equal(a.rows, b.rows) and int((a.rows[:, 0] > 0).sum()) == M
    assert zero_at_0 == M - slots and marked > 10


# ---------------------------------------------------------------------------------------------------------------- 5. Jerk_Primitive
def test_jerk_primitive_gives_zeros(pkg, hip):
    p = AC.params_of(pkg, 'Jerk-CVM')
    a, b = _env(hip, p, 4, swept_obs=True), _env(hip, p, 4)
    act = torch.full((4,), 0.5, dtype=torch.float64)
    for _ in range(10):
        oa, ob = a.step(act)[0], b.step(act)[0]
        assert oa['swep_map'].shape == oa['local_map'].shape and oa['swep_map'].dtype == torch.uint8 and not bool(oa['swep_map'].any())
        assert torch.equal(oa['local_map'], ob['local_map']) and bool(ob['local_map'].any())
        assert ob['swep_map'].data_ptr() == ob['local_map'].data_ptr()
    assert a.swept_map is None and a.swept_count is None


def test_the_library_refuses_what_it_cannot_hold(pkg, hip):
    """maps above 256 cells a side, at the constructor and again at the entry point"""
    import ctypes as C
    wide = pkg.Params(planner='Primitive', map_size=[2570, 500], agent_number=2, agent_radius=10, agent_max_speed=40, map_id=0)
    with pytest.raises(NotImplementedError, match=r'a map of 257 x 50 cells.*at most 256 x 256'):
        _env(hip, wide, 1, swept_obs=True)
    env = _env(hip, wide, 1)
    sw = A.Swept()
    one = torch.zeros(257 * 50, dtype=torch.uint8, device=env.device)
    for n in A.SWEPT_FIELDS:
        setattr(sw, n, one.data_ptr())
    assert hip.wpfn['swept_mark'](C.byref(env.cfg), C.byref(env._st), C.byref(env._plan), C.byref(sw), None) == -4
    assert b'256 x 256' in hip.fn['last_error']()
    assert hip.wpfn['swept_crop'](C.byref(env.cfg), C.byref(env._st), C.byref(sw), None) == -4
    assert hip.wpfn['swept_crop'](C.byref(env.cfg), C.byref(env._st), None, None) == -1
