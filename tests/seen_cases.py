"""The recorded time-since-observed maps (tests/golden/seen_episodes.npz, written by tests/golden/make_seen_golden.py) and the
comparisons tests/test_seen_obs_cpu.py (the model backend of tests/seen_backend.py) and tests/test_gpu_seen_obs.py (the HIP library)
share.  Every comparison is exact: integers, and the bit patterns of float32 / float64.  Test infrastructure."""
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seen_episodes.npz')
EPISODES = 4


@functools.lru_cache(maxsize=None)
def episode(i):
    z = np.load(PATH)
    pre = f'e{i}_'
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    d['cfg'] = json.loads(str(d['cfg']))
    return d


def params_of(pkg, ep, **kw):
    cfg = {k: v for k, v in ep['cfg'].items() if k != 'seed'}
    return pkg.Params(**dict(dict(planner='Primitive'), **dict(cfg, **kw)))


def bits(a):
    """the bit patterns of a float array (or the integers themselves): NaNs and signed zeros compare as what they are"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def never_value(ep, pkg):
    """[T]: what a never-seen cell holds in entry t of the episode (the table's second row at call t + 1)"""
    from drone2d_amd.device_plugins import tobs_table
    return tobs_table(params_of(pkg, ep))[1][1:len(ep['action']) + 1]


def refreshed_of(maps):
    """[T]: the cells entry t sees (value 0) that entry t - 1 did not -- never seen, or last seen two or more calls ago"""
    now = maps == 0
    return np.array([int(now[0].sum())] + [int((now[t] & ~now[t - 1]).sum()) for t in range(1, len(maps))])


@functools.lru_cache(maxsize=None)
def coverage():
    """(cells seen again after a gap of two or more calls, steps whose crop lies wholly inside the map, never-seen cells inside a
    crop) of the stored set"""
    import drone2d_amd as pkg
    reseen = inside = never = 0
    for i in range(EPISODES):
        ep = episode(i)
        p = params_of(pkg, ep)
        maps, nv = ep['map'], never_value(ep, pkg)
        T, W, H = maps.shape
        edge = 2 * (p.drone_view_depth // p.map_scale)
        now = maps == 0
        for t in range(T):
            if t:
                reseen += int((now[t] & ~now[t - 1] & (maps[t - 1] < nv[t - 1])).sum())
            ci, cj = int(ep['pose'][t, 0] // p.map_scale), int(ep['pose'][t, 1] // p.map_scale)
            inside += int(ci - edge >= 0 and ci + edge < W and cj - edge >= 0 and cj + edge < H)
            win = maps[t, max(ci - edge, 0): ci + edge + 1, max(cj - edge, 0): cj + edge + 1]
            never += int((win == nv[t]).sum())
    return reseen, inside, never


def check_env(env, ep, t, obs=None):
    """env 0 has taken `t` steps of the episode: its map is entry t of the recording, bit for bit, and so are the crop and the count"""
    import seen_model as SM
    env.sync()
    want = ep['map'][t]
    assert np.array_equal(bits(env.seen_age[0].cpu().numpy()), bits(want)), (t, int((bits(env.seen_age[0].cpu().numpy()) != bits(want)).sum()))
    sn = env.seen_calls[0].cpu().numpy()
    assert sn.dtype == np.int32 and np.array_equal(sn == t + 1, want == 0) and sn.max() <= t + 1 and sn.min() >= 0, t
    obs = env._result()[0] if obs is None else obs
    got = obs['age_map']
    L = env.cfg.L
    assert tuple(got.shape) == (1, 1, L, L) and str(got.dtype) == 'torch.float32'
    crop = SM.crop(want, ep['pose'][t, 0], ep['pose'][t, 1], L, env.cfg.scale)
    assert np.array_equal(bits(got[0, 0].cpu().numpy()), bits(crop)), t
    if 'refreshed' not in ep:
        ep['refreshed'] = refreshed_of(ep['map'])
    assert int(env.refreshed[0]) == int(ep['refreshed'][t]), (t, int(env.refreshed[0]), int(ep['refreshed'][t]))
    d = env.state.drone[0].cpu().numpy()
    assert np.array_equal(bits(d[:3]), bits(ep['pose'][t])), (t, d[:3].tolist(), ep['pose'][t].tolist())


def replay(env, ep, step):
    """the episode's recorded actions through `step(env, action)`, one env: before any step and after every step but the last the
    env shows the recording's next entry.  Returns the steps taken"""
    import torch
    from drone2d_amd import _abi as A
    T = len(ep['action'])
    check_env(env, ep, 0)
    for t in range(T):
        assert not bool(env.state.flags[0, A.F_DONE]), t
        step(env, torch.tensor([float(ep['action'][t])], dtype=torch.float64))
        if t + 1 < T:
            check_env(env, ep, t + 1)
    assert bool(env.state.flags[0, A.F_DONE])
    return T


# ---------------------------------------------------------------------------------------------------------------- handmade poses
POISON = 0xAB


def handmade_sets(pkg):
    """[(Params, view range, poses)]: per pose x, y, yaw, the steps taken, the call of the latest update (`last`) and whether the
    env's records are a plausible history (calls below this one) or poison.  Set 0, the default 50 x 50 map, 16 envs: the drone in
    every corner and on every edge (the view box and the crop clipped on each side), exactly on a cell's origin with yaw 0 / 90 / 180
    / 270 and 45 (cells on the cone's edge and on its axis, where the literal arccos decides), a pose off the grid, an env whose
    latest update already was this call (a finished env: nothing may be written) and one whose call lies beyond the table.  Sets 1
    and 2: maps of 30 x 20 and 20 x 30 cells.  Sets 3 and 4: drone_view_depth 45 with a 60 and a 120 degree view"""
    from drone2d_amd.device_plugins import tobs_table
    base = dict(planner='NoMove', agent_number=2, agent_radius=10, agent_max_speed=40, map_id=0)
    P = lambda x, y, yaw, steps=0, last=0, history=False: dict(x=x, y=y, yaw=yaw, steps=steps, last=last, history=history)   # noqa: E731
    p0 = pkg.Params(**base)
    n = tobs_table(p0).shape[1]
    set0 = [P(0.0, 0.0, 315.0), P(499.5, 0.0, 225.0, 3, 3, True), P(0.0, 499.5, 45.0, 17, 9), P(499.5, 499.5, 135.0, n - 2, 0, True),
            P(250.0, 0.0, 270.0, 4, 4, True), P(250.0, 499.9, 90.0, 1, 1), P(0.0, 250.0, 0.0, 2, 2, True), P(499.9, 250.0, 180.0, 60, 60, True),
            P(250.0, 250.0, 0.0, 5, 5, True), P(250.0, 250.0, 90.0), P(250.0, 250.0, 180.0, 8, 8, True), P(250.0, 250.0, 270.0, 9, 3),
            P(250.0, 250.0, 45.0, 30, 30, True), P(123.456, 321.987, 33.3, 12, 12, True),
            P(250.0, 250.0, 10.0, 5, 6), P(250.0, 250.0, 10.0, n - 1, 0, True)]      # (the finished env: all poison, and it stays so)
    assert len(set0) == 16
    small = [P(0.0, 0.0, 300.0), P(150.0, 100.0, 45.0, 6, 6, True), P(299.0, 199.0, 135.0, 2, 2), P(100.0, 199.0, 90.0, 7, 7, True),
             P(199.0, 100.0, 180.0, 3, 3, True), P(60.0, 60.0, 0.0, 4, 4, True)]
    short = [P(250.0, 250.0, 0.0, 3, 3, True), P(250.0, 250.0, 30.0), P(250.0, 250.0, 60.0, 5, 5, True), P(22.0, 478.0, 200.0, 9, 9, True),
             P(255.0, 245.0, 300.0, 2, 2), P(40.0, 40.0, 330.0, 11, 11, True)]
    wide = dict(base, map_size=[300, 200], init_pos=[50, 50], target_list=[[250, 150]])
    tall = dict(base, map_size=[200, 300], init_pos=[50, 50], target_list=[[150, 250]])
    return [(p0, 90, set0), (pkg.Params(**wide), 90, small), (pkg.Params(**tall), 90, [dict(q, x=q['y'], y=q['x']) for q in small]),
            (pkg.Params(**dict(base, drone_view_depth=45, drone_view_range=60)), 60, short),
            (pkg.Params(**dict(base, drone_view_depth=45, drone_view_range=120)), 120, short)]


def run_handmade(env, view_range, poses, launch, record=None):
    """The poses through `launch()` -- one d2d_seen_update over the env's own structs -- with every buffer the launch may write
    poisoned first, against the model; then a second launch without a step, which must change nothing.  Returns (envs left alone,
    cells marked, cells refreshed).  `record`: a list that receives the call's inputs and its checked outputs"""
    import torch
    import seen_model as SN
    from drone2d_amd import _abi as A
    B, cfg = len(poses), env.cfg
    assert env.num_envs == B
    tab = env.seen['tab'].cpu().numpy()
    rs = np.random.RandomState(3)
    drone, counters = env.state.drone.cpu().numpy().copy(), env.state.counters.cpu().numpy().copy()
    poison32 = int(np.full(4, POISON, dtype=np.uint8).view(np.int32)[0])
    seen = np.full((B, cfg.W, cfg.H), poison32, dtype=np.int32)
    last, refreshed = np.zeros(B, dtype=np.int32), np.full(B, poison32, dtype=np.int32)
    obs = np.frombuffer(np.full(B * cfg.L * cfg.L * 4, POISON, dtype=np.uint8).tobytes(), dtype=np.float32).reshape(B, cfg.L, cfg.L).copy()
    for e, q in enumerate(poses):
        drone[e, A.D_X], drone[e, A.D_Y], drone[e, A.D_YAW] = q['x'], q['y'], q['yaw']
        counters[e, A.C_STEPS], last[e] = q['steps'], q['last']
        if q['history']:
            seen[e] = rs.randint(0, q['steps'] + 1, size=(cfg.W, cfg.H))       # calls 0 .. steps: all below this call
    dev = env.device
    for t, v in ((env.state.drone, drone), (env.state.counters, counters), (env.seen['seen'], seen), (env.seen['last_call'], last),
                 (env.seen['refreshed'], refreshed), (env.seen['obs'], obs)):
        t.copy_(torch.from_numpy(v).to(dev))
    launch()
    env.sync()
    got = {k: env.seen[k].cpu().numpy() for k in ('seen', 'last_call', 'refreshed', 'obs')}
    alone = marked = fresh = 0
    want_seen = seen.copy()
    for e, q in enumerate(poses):
        out = SN.update(want_seen[e], last[e], q['steps'], (q['x'], q['y'], q['yaw']), cfg, view_range, tab)
        if out is None:
            assert np.array_equal(got['seen'][e], seen[e]) and got['last_call'][e] == last[e] and got['refreshed'][e] == poison32, e
            assert np.array_equal(bits(got['obs'][e]), bits(obs[e])), e
            alone += 1
            continue
        call, n, crop = out
        assert call == q['steps'] + 1 and got['last_call'][e] == call, e
        assert np.array_equal(got['seen'][e], want_seen[e]), (e, np.argwhere(got['seen'][e] != want_seen[e])[:5].tolist())
        assert got['refreshed'][e] == n, (e, int(got['refreshed'][e]), n)
        assert np.array_equal(bits(got['obs'][e]), bits(crop)), (e, np.argwhere(bits(got['obs'][e]) != bits(crop))[:5].tolist())
        outside = want_seen[e] != call
        assert np.array_equal(got['seen'][e][outside], seen[e][outside]), e      # cells outside the view keep what they held
        marked += int((~outside).sum())
        fresh += n
    launch()
    env.sync()
    for k in got:
        assert np.array_equal(bits(env.seen[k].cpu().numpy()), bits(got[k])), k
    if record is not None:
        record.append(dict(cfg=cfg, key_lo=env._seen.acos_key_lo, mask=env._seen.acos_mask, tab=tab, drone=drone, counters=counters,
                           seen=seen, last_call=last, refreshed=refreshed, obs=obs, want=got))
    return alone, marked, fresh


def check_call_1(env, e):
    """slot e is at step 0 of a world: its map is what the first plan() call leaves -- the start pose's view seen now, nothing else
    ever -- and so are the crop, the count and the call"""
    import seen_model as SN
    cfg, tab = env.cfg, env.seen['tab'].cpu().numpy()
    d = env.state.drone[e].cpu().numpy()
    view = SN.view_map(d[0], d[1], d[2], cfg.W, cfg.H, cfg.scale, float(cfg.depth), env.params.drone_view_range)
    assert view.any() and not view.all()
    assert np.array_equal(env.seen_calls[e].cpu().numpy(), view.astype(np.int32)), e
    assert int(env.seen['last_call'][e]) == 1 and int(env.refreshed[e]) == int(view.sum()), e
    age = SN.age_map(view.astype(np.int32), 1, tab)
    assert np.array_equal(bits(env.seen_age[e].cpu().numpy()), bits(age)), e
    assert np.array_equal(bits(env._result()[0]['age_map'][e, 0].cpu().numpy()), bits(SN.crop(age, d[0], d[1], cfg.L, cfg.scale))), e


def stream_pair(make, p, slots, M, refill_every=4, limit=2000):
    """The stream with the channel against the stream without it, turn for turn and step for step: rows, terms, done, local_map and
    yaw_angle are equal; every refilled slot shows the call-1 map at its step 0; a finished slot keeps its map, crop and count until
    the turn.  make(p, slots, seen_obs) -> env.  Returns (refills, frozen slot-steps checked)"""
    import torch
    from action_stream_backend import policy
    a = make(p, slots, True).action_stream(M, refill_every=refill_every)
    b = make(p, slots, False).action_stream(M, refill_every=refill_every)
    assert a.env.seen is not None and b.env.seen is None
    for e in range(slots):
        check_call_1(a.env, e)
    info = a.result()[3]
    kept, refills, frozen, calls = {}, 0, 0, 0
    while a.finished_now() < M:
        assert calls < limit
        last = info['episode'].clone()
        turned = a.turn()
        assert b.turn() == turned
        obs, terms, done, info = a.result()
        a.env.sync()
        for e in range(slots):
            if int(info['episode'][e]) != int(last[e]) and int(info['episode'][e]) >= 0:     # refilled: step 0 of a fresh world
                assert turned and int(info['steps'][e]) == 0 and not bool(done[e])
                check_call_1(a.env, e)
                kept.pop(e, None)
                refills += 1
            elif e in kept:                                                                  # done, not yet refilled: as it ended
                assert bool(done[e])
                now = (a.env.seen_calls[e], obs['age_map'][e], a.env.refreshed[e], a.env.seen['last_call'][e])
                assert all(torch.equal(x, y) for x, y in zip(now, kept[e])), e
                frozen += 1
        act = policy(info['episode'], info['steps'])
        oa, ta, da, ia = a.step(act)
        ob, tb, db, ib = b.step(act)
        assert torch.equal(a.rows, b.rows) and torch.equal(da, db), calls
        assert sorted(set(ta) - set(tb)) == ['refreshed'] and sorted(set(oa) - set(ob)) == ['age_map']
        assert all(torch.equal(ta[k], tb[k]) for k in tb) and all(torch.equal(ia[k], ib[k]) for k in ia), calls
        assert torch.equal(oa['local_map'], ob['local_map']) and torch.equal(oa['yaw_angle'], ob['yaw_angle']), calls
        assert ta['refreshed'].data_ptr() == a.env.refreshed.data_ptr()
        a.env.sync()
        for e in range(slots):
            if bool(da[e]) and e not in kept and bool(ia['live'][e]):
                kept[e] = tuple(x.clone() for x in (a.env.seen_calls[e], oa['age_map'][e], a.env.refreshed[e], a.env.seen['last_call'][e]))
        info = ia
        calls += 1
    a.close(), b.close()
    assert torch.equal(a.rows, b.rows) and int((a.rows[:, 0] > 0).sum()) == M
    return refills, frozen
