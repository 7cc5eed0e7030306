"""The renderer on the device (include/d2d_render.h: libd2d_render.so): the display list against the reference's recorded draw calls
bit for bit, the frames against the numpy model of the stated rules pixel for pixel, the handmade lists through the raster hook, and
what the calls leave alone: the env's state, the bytes around their buffers, the rows of `out` they were not asked for."""
import copy
import warnings

import numpy as np
import pytest
import torch

import render_cases as RC
import render_model as RM
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu

POISON = 0xAB
GUARD = 4096
SMALL = dict(planner='Primitive', map_size=[200, 130], init_pos=[20, 20], target_list=[[180, 110]], agent_number=4, agent_radius=5,
             agent_max_speed=20, drone_max_speed=30, pillar_number=2, drone_view_depth=40, drone_view_range=120, map_id=3)


def _env(hip, p, B, **kw):
    from drone2d_amd import vec_env
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', p.planner)
    return vec_env.VecDrone2DEnv(p, B, backend=hip, **kw)


def _step(env, action):
    env._set_action(action)
    env._jerk_step(True) if env.jerk is not None else env._plugins_step()


def _host_list(lst, k):
    """slot k of a render_list() result as the arrays of the model's lists"""
    n = int(lst['count'][k])
    return dict(kind=lst['kind'][k, :n].cpu().numpy(), rgb=lst['rgb'][k, :n].cpu().numpy(), width=lst['width'][k, :n].cpu().numpy(),
                npts=lst['npts'][k, :n].cpu().numpy(), geom=lst['geom'][k, :n].cpu().numpy(), count=n)


def _small_env(pkg, hip, B=4, steps=12, layout='rowmajor', **kw):
    env = _env(hip, pkg.Params(**dict(SMALL, **kw)), B, grid_layout=layout)
    rs = np.random.RandomState(17)
    for t in range(steps):
        _step(env, torch.from_numpy(rs.uniform(-1, 1, B)).to(env.device))
    env.sync()
    return env


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('i', range(RC.EPISODES))
def test_the_display_list_is_the_reference_s_calls(pkg, hip, i):
    """the four recorded episodes replayed on the device under the recorded actions: at every recorded step render_list() holds the
    reference's calls in order -- count, kinds, colours, widths and every float64 as bits -- and the explored map is its cell layer;
    the whole record, the arc's edge directions included, is the model's byte for byte"""
    assert hip.supports_render
    ep = RC.episode(i)
    p = RC.params_of(pkg, ep)
    if p.planner == 'NoMove':
        from drone2d_amd import vec_env
        env = vec_env.VecDrone2DEnv(p, 1, backend=hip)
        step = lambda a: env.step(np.array([a]))                     # noqa: E731
    else:
        env = _env(hip, p, 1, **(dict(jerk_tie=RC.tie_table()) if p.planner == 'Jerk_Primitive' else {}))
        step = lambda a: _step(env, torch.tensor([a], dtype=torch.float64, device=env.device))      # noqa: E731
    f = 0
    for t, a in enumerate(ep['action']):
        step(float(a))
        if f < len(ep['frame_step']) and int(ep['frame_step'][f]) == t + 1:
            lst = env.render_list()
            env.sync()
            assert lst['status'].tolist() == [A.RENDER_OK]
            got = _host_list(lst, 0)
            RC.assert_list_is(got, RC.frame_calls(ep, f), (i, f))
            want = RC.model_list(env, 0)
            assert np.array_equal(RC.to_bytes(got, got['count']), RC.to_bytes(want, want['count'])), (i, f)
            assert np.array_equal(RC.COLOUR_INDEX[RC.dmap_of(env, 0)], ep['cells'][f]), (i, f)
            f += 1
    assert f == len(ep['frame_step']) and bool(env.state.flags[0, A.F_DONE])
    # a finished slot renders its terminal state: a further call gives the same list, and a frame of the model's pixels
    again = _host_list(env.render_list(), 0)
    assert np.array_equal(RC.to_bytes(again, again['count']), RC.to_bytes(got, got['count']))
    frame = env.render_frames(downsample=2)
    env.sync()
    assert np.array_equal(frame[0].cpu().numpy(), RM.raster(got, RC.dmap_of(env, 0), p.map_size[0], p.map_size[1], p.map_scale, 2))


# ---------------------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize('layout', ['rowmajor', 'tiled'])
def test_frames_are_the_model_s_raster_of_the_device_s_own_list(pkg, hip, layout):
    """a 200 x 130 px map (20 x 13 cells, ragged against the 128 x 32 tile and the 16-pixel run), 4 slots 12 steps in, all pixels:
    downsample 1, 2 and 3, the slots in a shuffled order with a repeat, one slot alone; frames[k] of a subset is the all-slots frame"""
    env = _small_env(pkg, hip, layout=layout)
    assert (env.cfg.W, env.cfg.H, env.cfg.grid_tile) == (20, 13, 16 if layout == 'tiled' else 0) and env.state.pillars.shape[1] == 2
    lst = env.render_list()
    env.sync()
    lists = [_host_list(lst, e) for e in range(4)]
    assert all(int(l['count']) >= A.render_cap(2, 4, 0) for l in lists) and any(int(l['count']) > A.render_cap(2, 4, 0) for l in lists)
    for e in range(4):                                          # the list is the model's of the slot's state
        want = RC.model_list(env, e)
        assert np.array_equal(RC.to_bytes(lists[e], lists[e]['count']), RC.to_bytes(want, want['count'])), e
    for d in (1, 2, 3):
        whole = env.render_frames(downsample=d)
        assert tuple(whole.shape) == (4, -(-130 // d), -(-200 // d), 3) and whole.dtype == torch.uint8 and whole.device.type == 'cuda'
        whole = whole.cpu().numpy()
        for e in range(4):
            want = RM.raster(lists[e], RC.dmap_of(env, e), 200, 130, 10, d)
            assert np.array_equal(whole[e], want), (d, e, np.argwhere(whole[e] != want)[:5].tolist())
        assert len({w.tobytes() for w in whole}) == 4           # four worlds, four pictures
        order = [2, 0, 3, 0, 1]
        for slots in (order, torch.tensor(order, device=env.device), torch.tensor(order, dtype=torch.int32, device=env.device), [3]):
            sub = env.render_frames(slots, downsample=d).cpu().numpy()
            idx = slots.tolist() if isinstance(slots, torch.Tensor) else slots
            assert len(sub) == len(idx) and all(np.array_equal(sub[k], whole[e]) for k, e in enumerate(idx))
    full = env.render_frames().cpu().numpy()
    assert np.array_equal(env.render_frames(downsample=3).cpu().numpy(), full[:, ::3, ::3])
    assert {100, 200, 240} <= set(np.unique(full[..., 0]).tolist()) and (full == 0).all(axis=3).any()     # cells of all kinds, a black polyline


# ---------------------------------------------------------------------------------------------------------------- 3. the hook
def _guarded(nbytes, device, offset=0):
    """(a poisoned uint8 buffer, the view of `nbytes` at GUARD + offset inside it)"""
    big = torch.full((GUARD * 2 + nbytes + 64,), POISON, dtype=torch.uint8, device=device)
    return big, big[GUARD + offset:GUARD + offset + nbytes]


def _guards_intact(big, nbytes, offset=0):
    return bool((big[:GUARD + offset] == POISON).all()) and bool((big[GUARD + offset + nbytes:] == POISON).all())


@pytest.mark.parametrize('offset', [0, 3])
def test_handmade_lists_through_the_raster_hook(pkg, hip, offset):
    """the cases of the host build on the device, by the same digests; the frame and the boxes lie inside poisoned buffers whose
    other bytes stay as they were.  offset 3: a frame that starts 3 bytes off a multiple of 16 takes the single-byte stores"""
    dev = hip.device
    for c in RC.handmade():
        n = int(c['list']['count'])
        cap = max(n, 1)
        d = c['d']
        Hf, Wf = -(-c['H_px'] // d), -(-c['W_px'] // d)
        items = torch.from_numpy(RC.to_bytes(c['list'], cap)).to(dev)
        count = torch.tensor([n], dtype=torch.int32, device=dev)
        cells = torch.from_numpy(np.ascontiguousarray(c['cells'])).to(dev)
        fbig, frame = _guarded(Hf * Wf * 3, dev, offset)
        bbig, bbox = _guarded(cap * 8, dev)
        r = A.RasterCall()
        r.items, r.count, r.cells, r.bbox, r.frame = items.data_ptr(), count.data_ptr(), cells.data_ptr(), bbox.data_ptr(), frame.data_ptr()
        r.S, r.cap, r.W, r.H, r.W_px, r.H_px, r.scale, r.downsample = 1, cap, c['W'], c['H'], c['W_px'], c['H_px'], c['scale'], d
        hip.render_raster(r)
        hip.sync()
        got = frame.cpu().numpy().reshape(Hf, Wf, 3)
        want = RC.model_frame(c)
        assert np.array_equal(got, want), (c['name'], np.argwhere(got != want)[:5].tolist())
        assert RC.digest(got) == RC.digest(want)
        assert _guards_intact(fbig, Hf * Wf * 3, offset) and _guards_intact(bbig, cap * 8), c['name']


def test_several_lists_in_one_raster_launch(pkg, hip):
    """S = 3 caller-made lists of different lengths under one cap, each over its own cell layer"""
    dev = hip.device
    cs = [c for c in RC.handmade() if c['name'] in ('corners', 'many', 'arcs')]
    cap = max(int(c['list']['count']) for c in cs)
    items = torch.from_numpy(np.stack([RC.to_bytes(c['list'], cap) for c in cs])).to(dev)
    count = torch.tensor([int(c['list']['count']) for c in cs], dtype=torch.int32, device=dev)
    cells = torch.from_numpy(np.stack([c['cells'] for c in cs])).to(dev)
    frame = torch.full((3, 130, 200, 3), POISON, dtype=torch.uint8, device=dev)
    bbox = torch.zeros((3, cap, 4), dtype=torch.int16, device=dev)
    r = A.RasterCall()
    r.items, r.count, r.cells, r.bbox, r.frame = items.data_ptr(), count.data_ptr(), cells.data_ptr(), bbox.data_ptr(), frame.data_ptr()
    r.S, r.cap, r.W, r.H, r.W_px, r.H_px, r.scale, r.downsample = 3, cap, 20, 13, 200, 130, 10, 1
    hip.render_raster(r)
    hip.sync()
    for k, c in enumerate(cs):
        assert np.array_equal(frame[k].cpu().numpy(), RC.model_frame(c)), c['name']


# ---------------------------------------------------------------------------------------------------------------- 4. it only reads
def test_rendering_writes_nothing_of_the_env(pkg, hip):
    env = _small_env(pkg, hip, steps=6)
    before = [(n, t.clone()) for n, t, _ in env.fork_items()]
    env.render_list()
    env.render_frames(downsample=2)
    env.render_frames([1, 1, 3])
    env.sync()
    now = {n: t for n, t, _ in env.fork_items()}
    assert len(before) > 20 and 'state.pillars' in now
    for n, t in before:
        assert torch.equal(t.reshape(-1).view(torch.uint8), now[n].reshape(-1).view(torch.uint8)), n
    # the scratch is no state: no item, no holder
    assert not any('render' in n for n in now)


def test_a_rendered_twin_stays_bit_equal(pkg, hip):
    """two envs of the same worlds under the same actions, one rendered after every step: equal in every tensor of state.t after 30"""
    p = pkg.Params(**dict(SMALL, max_flight_time=20))
    a, b = _env(hip, p, 3), _env(hip, p, 3)
    rs = np.random.RandomState(23)
    for t in range(30):
        act = torch.from_numpy(rs.uniform(-1, 1, 3)).to(a.device)
        _step(a, act)
        _step(b, act)
        a.render_frames(downsample=1 + t % 3)
        a.render_list([2, 0])
    a.sync(), b.sync()
    for k in a.state.t:
        assert torch.equal(a.state.t[k].reshape(-1).view(torch.uint8), b.state.t[k].reshape(-1).view(torch.uint8)), k
    for k in a.plugins.t:
        if k != 'launch_args':
            assert torch.equal(a.plugins.t[k].reshape(-1).view(torch.uint8), b.plugins.t[k].reshape(-1).view(torch.uint8)), k
    assert int(a.state.counters[:, 0].max()) == 30


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
def test_the_buffers_edges_and_the_rows_not_asked_for(pkg, hip):
    from drone2d_amd import render
    env = _small_env(pkg, hip, steps=8)
    dev = env.device
    S, cap = 3, A.render_cap(2, 4, int(env.plugins.t['traj'].shape[1]))
    # the list buffers inside poisoned ones
    sc = render.RenderScratch()
    sizes = dict(items=S * cap * A.RENDER_ITEM_BYTES, bbox=S * cap * 8, count=S * 4, status=S)
    big = {}
    for name, nbytes in sizes.items():
        big[name], view = _guarded(nbytes, dev)
        setattr(sc, name, view.view({'items': torch.uint8, 'bbox': torch.int16, 'count': torch.int32, 'status': torch.uint8}[name]).reshape(
            {'items': (S, cap, A.RENDER_ITEM_BYTES), 'bbox': (S, cap, 4), 'count': (S,), 'status': (S,)}[name]))
    sc.key = (S, cap)
    env._render = sc
    # ... and the frame: 5 rows of `out`, 3 asked for
    Hf, Wf = 130, 200
    fbig, fview = _guarded(5 * Hf * Wf * 3, dev)
    out = fview.view(5, Hf, Wf, 3)
    got = env.render_frames([3, 0, 3], out=out)
    env.sync()
    assert env._render is sc and got.data_ptr() == out.data_ptr() and tuple(got.shape) == (3, Hf, Wf, 3)
    assert all(_guards_intact(big[n], sizes[n]) for n in sizes) and _guards_intact(fbig, 5 * Hf * Wf * 3)
    assert bool((out[3:] == POISON).all()) and sc.status.tolist() == [0, 0, 0]
    # the rows of the list beyond a slot's count are left alone
    n0 = int(sc.count[0])
    assert n0 < cap and bool((sc.items[0, n0:] == POISON).all()) and bool((sc.bbox.view(torch.uint8).reshape(S, cap, 8)[0, n0:] == POISON).all())
    whole = env.render_frames().cpu().numpy()                   # (another size: the scratch is allocated anew)
    assert all(np.array_equal(got[k].cpu().numpy(), whole[e]) for k, e in enumerate([3, 0, 3]))
    # a capacity made too small by hand, under trajectories of 0, 3, 40 and 1 positions: the slot whose list does not fit says so
    # and draws nothing but its cells
    mine = [np.zeros((0, 2)), np.array([[10.0, 10.0], [50.5, 60.25], [120.0, 20.0]]), np.linspace([5.0, 5.0], [190.0, 120.0], 40), np.ones((1, 2))]
    mixed = env.render_frames(trajectories=mine).cpu().numpy()
    counts = render.lists(env, trajectories=mine)['count'].tolist()
    small = A.render_cap(2, 4, 3)
    assert counts == [small - 2, small, small + 37, small - 2]
    lst = render.lists(env, trajectories=mine, cap=small)
    env.sync()
    fits = [c <= small for c in counts]
    assert lst['status'].tolist() == [A.RENDER_OK if ok else A.RENDER_OVERFLOW for ok in fits]
    assert lst['count'].tolist() == [c if ok else 0 for c, ok in zip(counts, fits)]
    fr = render.frames(env, trajectories=mine, cap=small).cpu().numpy()
    for e, ok in enumerate(fits):
        want = mixed[e] if ok else RM.cell_layer(RC.dmap_of(env, e), 200, 130, 10)
        assert np.array_equal(fr[e], want), e
    # a slot outside the batch, which only a tensor can name: nothing of it is read, its frame is blank
    odd = env.render_frames(torch.tensor([1, 99, -1], device=dev)).cpu().numpy()
    assert np.array_equal(odd[0], whole[1]) and (odd[1:] == 240).all()


# ---------------------------------------------------------------------------------------------------------------- 6. the pillars follow a slot
def _pillar_discs(env, e, lst=None):
    lst = env.render_list() if lst is None else lst
    env.sync()
    P = env.state.pillars.shape[1]
    g = lst['geom'][e, 9:9 + P, :3].cpu().numpy()
    assert (lst['kind'][e, 9:9 + P] == A.RK_DISC).all() and (lst['rgb'][e, 9:9 + P] == 130).all()
    return g


def test_a_slot_s_pillars_follow_it(pkg, hip):
    """an action stream of 4 slots over 12 seeded episodes (CVM: the pillars are resident without RVO): after every refill the slot's
    pillar discs are those of the world with its new map id, as host_init builds it; load_slots() carries them into a sibling"""
    from drone2d_amd import host_init
    p = pkg.Params(planner='Jerk_Primitive', agent_number=6, agent_radius=10, agent_max_speed=20, pillar_number=3, max_flight_time=1.5, map_id=40)
    env = _env(hip, p, 4, worlds='device')
    assert not env.rvo and tuple(env.state.pillars.shape) == (4, 3, 3)
    stream = env.action_stream(12, refill_every=1)
    act = torch.full((4,), 0.25, dtype=torch.float64, device=env.device)
    seen, calls = set(), 0
    while stream.finished_now() < 12 and calls < 400:
        obs, terms, done, info = stream.step(act)
        calls += 1
        if calls % 4 == 0 or stream.finished_now() >= 8:
            eps = info['episode'].tolist()
            lst = env.render_list()
            for e, k in enumerate(eps):
                if k < 0 or (e, k) in seen:
                    continue
                q = copy.copy(p)
                q.map_id = p.map_id + k
                want = np.asarray(host_init.init_world(q)['obstacles'], dtype=np.float64).reshape(-1, 3)
                assert np.array_equal(_pillar_discs(env, e, lst), want), (e, k)
                seen.add((e, k))
        if calls == 30:                      # mid-stream: a sibling loads the slots crosswise, pillars included
            sib = env.sibling(4)
            src = torch.tensor([3, 2, 1, 0], dtype=torch.int32, device=env.device)
            assert sib.load_slots(env, src).tolist() == [1, 1, 1, 1]
            assert np.array_equal(np.stack([_pillar_discs(sib, e) for e in range(4)]), np.stack([_pillar_discs(env, 3 - e) for e in range(4)]))
            assert np.array_equal(sib.render_frames(downsample=4).cpu().numpy(), env.render_frames([3, 2, 1, 0], downsample=4).cpu().numpy())
    stream.close()
    assert stream.finished_now() == 12 and len({k for _, k in seen}) >= 8 and calls >= 30


# ---------------------------------------------------------------------------------------------------------------- 7. the facade
def test_the_facade_renders_its_one_env(pkg, hip):
    from drone2d_amd import env as envmod
    p = pkg.Params(planner=RC.straight_planner(), agent_number=6, agent_radius=10, agent_max_speed=20, drone_max_speed=40, map_id=2)
    e = envmod.Drone2DEnv2(p, backend=hip)
    for t in range(8):
        e.step(0.3)
    arr = e.render('rgb_array')
    assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and arr.shape == (p.map_size[1], p.map_size[0], 3)
    assert e._mode == 'host'                                    # a host planner: its stored trajectory is uploaded with the call
    traj = [np.asarray(e.planner.trajectory.positions, dtype=np.float64).reshape(-1, 2)]
    assert len(traj[0]) > 1
    assert np.array_equal(arr, e._vec.render_frames([0], trajectories=traj)[0].cpu().numpy())
    lst = _host_list(e._vec.render_list([0], trajectories=traj), 0)
    assert np.array_equal(arr, RM.raster(lst, RC.dmap_of(e._vec, 0), p.map_size[0], p.map_size[1], p.map_scale))
    assert (arr == 0).all(axis=2).any()                          # the stored trajectory, in black
    # the device planner's trajectory needs no upload
    q = pkg.Params(planner='Primitive', agent_number=6, agent_radius=10, agent_max_speed=20, drone_max_speed=40, map_id=2)
    dv = envmod.Drone2DEnv2(q, backend=hip)
    for t in range(8):
        dv.step(0.3)
    assert dv._mode == 'device' and np.array_equal(dv.render('rgb_array'), dv._vec.render_frames([0])[0].cpu().numpy())
    assert (dv.render('rgb_array') == 0).all(axis=2).any()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert e.render() is None and e.render('human') is None and e.render(mode='human') is None
    assert len(seen) == 1 and 'headless' in str(seen[0].message)
