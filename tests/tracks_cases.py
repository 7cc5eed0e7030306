"""The recorded tracker states and forecast windows (tests/golden/tracks_episodes.npz, written by tests/golden/make_tracks_golden.py),
the handmade single-env cases, and the comparisons tests/test_tracks_obs_cpu.py (the model backend of tests/tracks_backend.py, the host
build of csrc/tracks/d2d_tracks.h) and tests/test_gpu_tracks_obs.py (the HIP library) share.  Every comparison is exact equality of
integers.  Test infrastructure."""
import ctypes as C
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tracks_episodes.npz')
EPISODES = 4
SAMPLES = 31
POISON = 0xAB
POISON32 = int(np.full(4, POISON, dtype=np.uint8).view(np.int32)[0])


@functools.lru_cache(maxsize=None)
def episode(i):
    z = np.load(PATH)
    pre = f'e{i}_'
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    d['cfg'] = json.loads(str(d['cfg']))
    return d


@functools.lru_cache(maxsize=None)
def tie_table():
    z = np.load(PATH)
    return z['tie_perm'], z['tie_eq']


def params_of(pkg, ep, **kw):
    cfg = {k: v for k, v in ep['cfg'].items() if k != 'seed'}
    return pkg.Params(**dict(cfg, **kw))


def cfg_of(p, B, N):
    from drone2d_amd import host_init
    return host_init.derive_cfg(p, B=B, N=N)


def default_margin(p):
    return float(5 + p.var_cam)


@functools.lru_cache(maxsize=None)
def coverage():
    """(steps with a nonzero window, steps with two or more active trackers inside the window, steps with a cell two trackers reach
    at different samples, steps whose window overlaps the padding, steps with active trackers and an all-zero window) of the stored
    set"""
    import drone2d_amd as pkg
    import tracks_model as TM
    nonzero = two = shared = padded = empty = 0
    for i in range(EPISODES):
        ep = episode(i)
        p = params_of(pkg, ep)
        cfg = cfg_of(p, 1, ep['active'].shape[1])
        edge = (cfg.L - 1) // 2
        for t in range(len(ep['action'])):
            act, mu, win = ep['active'][t] != 0, ep['mu'][t], ep['win'][t]
            ci, cj = int(ep['pose'][t, 0] // p.map_scale), int(ep['pose'][t, 1] // p.map_scale)
            nonzero += int(win.any())
            empty += int(act.any() and not win.any())
            padded += int(ci - edge < 0 or ci + edge >= cfg.W or cj - edge < 0 or cj + edge >= cfg.H)
            ti, tj = mu[:, 0] // p.map_scale, mu[:, 1] // p.map_scale
            inside = act & (np.abs(ti - ci) <= edge) & (np.abs(tj - cj) <= edge)
            two += int(inside.sum() >= 2)
            if shared == 0 and inside.sum() >= 2:
                one = [TM.window(ep['pose'][t], mu, np.arange(len(act)) == q, ep['radius'][t], cfg, default_margin(p), SAMPLES)
                       for q in np.nonzero(act)[0]]
                for a in range(len(one)):
                    for b in range(a + 1, len(one)):
                        shared += int(((one[a] != 0) & (one[b] != 0) & (one[a] != one[b])).any())
    return nonzero, two, shared, padded, empty


def assert_coverage(cov):
    nonzero, two, shared, padded, empty = cov
    assert nonzero >= 100 and two >= 20 and shared >= 1 and padded >= 1 and empty >= 1, cov


# ---------------------------------------------------------------------------------------------------------------- the env
def env_tracks(env, e=0):
    """(pose, mu [N, 4], active [N], radius [N]) of env e as it stands"""
    N = env.cfg.N
    return (env.state.drone[e, :3].cpu().numpy(), env.state.kf[e].cpu().numpy().reshape(-1, env.state.kf.shape[-1])[:N, :4],
            env.state.active[e].cpu().numpy()[:N], env.tracks['trk_radius'][e].cpu().numpy()[:N])


def check_env(env, ep, t):
    """env 0 has taken t + 1 steps of the episode: the pose, the active flags and the radii are entry t of the recording, and the
    window, the observation and the count are the recorded window's, exactly.  The trackers' means are the step's own matter: its
    Kalman update orders the matrix products its own way, so a mean may differ from numpy's in its last bits (an ulp of a coordinate
    of this map is below 1e-13, and an episode has at most a hundred updates).  They are held to 1e-9 px and px / s here, far above
    any accumulated rounding and far below anything that moves a forecast by a cell; the windows below are compared exactly"""
    env.sync()
    pose, mu, active, radius = env_tracks(env)
    on = ep['active'][t] != 0
    assert np.array_equal(pose.view(np.uint64), ep['pose'][t].view(np.uint64)), (t, pose.tolist(), ep['pose'][t].tolist())
    assert np.array_equal(active != 0, on), t
    assert np.all(np.abs(mu[on] - ep['mu'][t][on]) <= 1e-9), (t, np.abs(mu[on] - ep['mu'][t][on]).max())
    assert np.array_equal(radius[on], ep['radius'][t][on]), (t, radius.tolist(), ep['radius'][t].tolist())
    check_window(env, ep['win'][t], t)


def check_window(env, want, t=None, e=0):
    L = env.cfg.L
    win, obs = env.track_win[e].cpu().numpy(), env._result()[0]['track_map']
    assert win.dtype == np.uint8 and np.array_equal(win, want), (t, np.argwhere(win != want)[:5].tolist())
    assert tuple(obs.shape) == (env.num_envs, 1, L, L) and str(obs.dtype) == 'torch.float32'
    assert np.array_equal(obs[e, 0].cpu().numpy(), want.astype(np.float32)), t
    assert int(env.track_cells[e]) == int((want != 0).sum()), t


def replay(env, ep, step, margin0=None):
    """the episode's recorded actions through `step(env, action)`, one env: zero before any step, the recording's entry after every
    step, the terminal one included.  `margin0`: an env of the same world built with tracks_margin=0, stepped alongside and compared
    every tenth step.  Returns the steps taken"""
    import torch
    from drone2d_amd import _abi as A
    T = len(ep['action'])
    envs = [env] + ([margin0] if margin0 is not None else [])
    for e_ in envs:
        e_.sync()
        assert not bool(e_.track_win.any()) and int(e_.tracks['last_step'][0]) == 0
    for t in range(T):
        for e_ in envs:
            assert not bool(e_.state.flags[0, A.F_DONE]), t
            step(e_, torch.tensor([float(ep['action'][t])], dtype=torch.float64, device=e_.device))
        check_env(env, ep, t)
        if margin0 is not None and t % 10 == 0:
            margin0.sync()
            check_window(margin0, ep['win0'][t // 10], t)
    assert bool(env.state.flags[0, A.F_DONE]) and int(env.tracks['last_step'][0]) == T
    return T


# ---------------------------------------------------------------------------------------------------------------- handmade cases
def _env(x, y, trackers, steps=3, last=2):
    """one env: the drone's position, its step counter, the counter of its latest update, and per tracker (active, mx, my, vx, vy,
    radius)"""
    return dict(x=float(x), y=float(y), steps=int(steps), last=int(last), trackers=[tuple(t) for t in trackers])


def handmade_sets(pkg):
    """[dict(name, params, N, samples, margin, envs)]: every set is one launch of five envs -- one more than a block's waves -- that
    share a d2d_cfg.  thr = drone_radius + radius + margin = 10 + 10 + 5 = 25 px for the default radius and margin.

    near      N = 5, 31 samples, the 50 x 50 map, L = 33.  Two trackers that reach one cell at different samples (the smaller wins)
              next to an inactive tracker with a stale mu right on the drone; a forecast that leaves the map and one that starts
              outside the window and enters it; the drone in a corner (half the window is padding); a tracker exactly thr from a cell
              centre along x and another along y, and one an ulp further; an env whose latest update was at this counter (skipped)
    single    N = 1, one sample, margin 0: the disc of the latest mu alone; radii 3 and 17; a NaN mu; a tracker far outside the map
    crowd     N = 70 (more than one wave of trackers), 255 samples, a 25 x 19-cell map, L = 5 (drone_view_depth 10): seeded tracker
              states, 0, 1, 64, 65 and 70 of them active
    small     N = 5, 31 samples, the 25 x 19-cell map with L = 33 (the window is larger than the map), margin 0
    none      N = 0: no tracker buffers at all, zeros"""
    base = dict(planner='Primitive', agent_number=5, agent_radius=10, agent_max_speed=40, map_id=0)
    T = lambda on, mx, my, vx=0.0, vy=0.0, r=10.0: (on, mx, my, vx, vy, r)       # noqa: E731
    off = T(0, 1e3, 1e3)
    near = [
        _env(250, 250, [T(1, 200, 255, 40, 0), T(1, 255, 330, 0, -40), T(0, 250, 250, 0, 0, 17), off, off]),
        _env(400, 250, [T(1, 470, 250, 60, 0), T(1, 150, 250, 50, 10), T(1, 405, 30, 0, 45), off, off], steps=7, last=3),
        _env(5, 5, [T(1, 30, 20, -20, 5), T(1, 10, 160, 0, -30), off, off, T(1, 120, 8, 10, 0)], steps=1, last=0),
        # (cell centres are at 10 i + 5: (255, 255) is 25 px from the first, (195, 175) from the second, (105, 115) an ulp more from the third)
        _env(255, 255, [T(1, 280, 255), T(1, 195, 150), T(1, 105, float(np.nextafter(140.0, 141.0))), off, off], steps=9, last=-1),
        _env(250, 250, [T(1, 250, 250, 10, 10), off, off, off, off], steps=4, last=4),
    ]
    single = [
        _env(250, 250, [T(1, 262, 239, 99, 99, 3)]), _env(250, 250, [T(1, 262, 239, 99, 99, 17)]),
        _env(250, 250, [T(1, float('nan'), 250, 1, 1)]), _env(499, 0, [T(1, 1e6, -1e6, -1, 1)]), _env(250, 250, [T(0, 250, 250)], steps=2, last=2),
    ]
    rs = np.random.RandomState(11)
    crowd = []
    for n_on in (0, 1, 64, 65, 70):
        on = np.zeros(70, dtype=int)
        on[rs.permutation(70)[:n_on]] = 1
        trk = [T(int(on[q]), rs.uniform(-20, 270), rs.uniform(-20, 210), rs.uniform(-40, 40), rs.uniform(-40, 40), rs.uniform(3, 17)) for q in range(70)]
        crowd.append(_env(rs.uniform(1, 249), rs.uniform(1, 189), trk, steps=n_on, last=n_on - 1))
    small = [
        _env(125, 95, [T(1, 30, 30, 30, 20), T(1, 240, 180, -35, -25), off, off, off]),
        _env(0, 0, [T(1, 5, 5, 10, 10), off, off, off, off]), _env(249, 189, [T(1, 245, 185, -10, -10), off, off, off, off]),
        _env(249, 0, [T(1, 125, 95, 40, -40), T(1, 125, 95, -40, 40), off, off, off]), _env(60, 150, [off, off, off, off, T(1, 60, 150, 0, 0, 17)]),
    ]
    tiny = dict(base, map_size=[250, 190], init_pos=[50, 50], target_list=[[200, 150]])
    sets = [dict(name='near', params=pkg.Params(**base), N=5, samples=31, margin=5.0, envs=near),
            dict(name='single', params=pkg.Params(**base), N=1, samples=1, margin=0.0, envs=single),
            dict(name='crowd', params=pkg.Params(**dict(tiny, drone_view_depth=10)), N=70, samples=255, margin=5.0, envs=crowd),
            dict(name='small', params=pkg.Params(**tiny), N=5, samples=31, margin=0.0, envs=small),
            dict(name='none', params=pkg.Params(**base), N=0, samples=31, margin=5.0,
                 envs=[_env(250, 250, []), _env(0, 0, []), _env(499, 499, [], steps=5, last=5), _env(10, 400, []), _env(300, 20, [])])]
    for s in sets:
        assert len(s['envs']) == 5 and all(len(q['trackers']) == s['N'] for q in s['envs']), s['name']
    return sets


def pack(hs, device='cpu'):
    """The set as the structs of one launch over torch tensors on `device`, every buffer the launch may write poisoned.  Returns
    (cfg, st, tracks, tensors): keep `tensors` alive as long as the structs are used"""
    import torch
    from drone2d_amd import _abi as A
    B, N = len(hs['envs']), hs['N']
    cfg = cfg_of(hs['params'], B, N)
    drone, counters = np.zeros((B, A.DF)), np.zeros((B, A.CF), dtype=np.int32)
    kf = np.frombuffer(np.full(B * N * A.KF * 8, 0x7f, dtype=np.uint8).tobytes(), dtype=np.float64).reshape(B, N, A.KF).copy()   # (NaNs beyond mu)
    active, radius, last = np.zeros((B, N), dtype=np.uint8), np.zeros((B, N)), np.zeros(B, dtype=np.int32)
    for e, q in enumerate(hs['envs']):
        drone[e, A.D_X], drone[e, A.D_Y], counters[e, A.C_STEPS], last[e] = q['x'], q['y'], q['steps'], q['last']
        for k, (on, mx, my, vx, vy, r) in enumerate(q['trackers']):
            active[e, k], radius[e, k] = on, r
            kf[e, k, :4] = mx, my, vx, vy
    t = dict(drone=drone, counters=counters, kf=kf, active=active, trk_radius=radius, last_step=last,
             win=np.full((B, cfg.L, cfg.L), POISON, dtype=np.uint8), cells=np.full(B, POISON32, dtype=np.int32))
    t = {k: torch.from_numpy(v).to(device) for k, v in t.items()}
    st, tr = A.State(), A.Tracks()
    for n in ('drone', 'counters', 'kf', 'active'):
        setattr(st, n, t[n].data_ptr())
    for n in A.TRACKS_POINTERS:
        setattr(tr, n, t[n].data_ptr())
    tr.margin, tr.samples, tr.force = hs['margin'], hs['samples'], 0
    return cfg, st, tr, t


def run_handmade(hs, launch, device='cpu', sync=lambda: None, record=None):
    """The set through `launch(cfg, st, tracks)` -- one d2d_tracks_update -- over poisoned outputs, against the model; a second launch,
    which must change nothing; then the same with `force`, which updates the skipped envs too.  Returns (envs the first launch left
    alone, nonzero cells of the forced windows).  `record`: a list that receives the launches' inputs and checked outputs"""
    import tracks_model as TM
    cfg, st, tr, t = pack(hs, device)
    before = {k: t[k].cpu().numpy().copy() for k in ('win', 'cells', 'last_step')}
    pose = t['drone'].cpu().numpy()
    mu, active, radius = t['kf'].cpu().numpy()[:, :, :4], t['active'].cpu().numpy(), t['trk_radius'].cpu().numpy()
    steps = t['counters'].cpu().numpy()[:, 0]

    def want_of(force, prev):
        want = {k: v.copy() for k, v in prev.items()}
        for e in range(cfg.B):
            out = TM.update(None, None, prev['last_step'][e], steps[e], pose[e], mu[e], active[e], radius[e], cfg, hs['margin'],
                            hs['samples'], force)
            if out is not None:
                want['win'][e], want['cells'][e], want['last_step'][e] = out
        return want

    def check(want, what):
        sync()
        for k in want:
            got = t[k].cpu().numpy()
            assert np.array_equal(got, want[k]), (hs['name'], what, k, np.argwhere(got != want[k])[:5].tolist())
    first = want_of(0, before)
    alone = int(sum(np.array_equal(first['win'][e], before['win'][e]) for e in range(cfg.B)))
    launch(cfg, st, tr)
    check(first, 'first')
    launch(cfg, st, tr)
    check(first, 'repeat')
    forced = want_of(1, first)
    tr.force = 1
    launch(cfg, st, tr)
    check(forced, 'forced')
    assert not (forced['win'] == POISON).all(axis=(1, 2)).any() and (forced['last_step'] == steps).all()
    if record is not None:
        record.append(dict(cfg=cfg, hs=hs, inputs={k: t[k].cpu().numpy() for k in ('drone', 'counters', 'kf', 'active', 'trk_radius')},
                           before=before, first=first, forced=forced))
    return alone, int((forced['win'] != 0).sum())


def expected_handmade(name):
    """the envs of the set whose counter equals that of their latest update: those the first launch leaves alone"""
    return {'near': 1, 'single': 1, 'crowd': 0, 'small': 0, 'none': 1}[name]


# ---------------------------------------------------------------------------------------------------------------- streams
def stream_pair(make, p, slots, M, refill_every=4, limit=2000):
    """The stream with the channel against the stream without it, turn for turn and step for step: rows, terms, done and the other
    observations are equal; the window is the model's of the slot's own state after every step; a refilled slot shows zeros at its
    step 0; a finished slot keeps its window until the turn.  make(p, slots, tracks_obs) -> env.  Returns (refills, frozen
    slot-steps checked, nonzero windows seen)"""
    import torch
    import tracks_model as TM
    from action_stream_backend import policy
    a = make(p, slots, True).action_stream(M, refill_every=refill_every)
    b = make(p, slots, False).action_stream(M, refill_every=refill_every)
    assert a.env.tracks is not None and b.env.tracks is None
    info = a.result()[3]
    kept, refills, frozen, nonzero, calls = {}, 0, 0, 0, 0
    margin, samples = a.env._tracks.margin, a.env._tracks.samples
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
                assert not bool(obs['track_map'][e].any()) and int(terms['track_cells'][e]) == 0 and int(a.env.tracks['last_step'][e]) == 0
                kept.pop(e, None)
                refills += 1
            elif e in kept:                                                                  # done, not yet refilled: as it ended
                assert bool(done[e])
                now = (a.env.track_win[e], obs['track_map'][e], a.env.track_cells[e], a.env.tracks['last_step'][e])
                assert all(torch.equal(x, y) for x, y in zip(now, kept[e])), e
                frozen += 1
        act = policy(info['episode'], info['steps'])
        was_live = ~a.env.state.flags[:, 3].bool().clone()
        oa, ta, da, ia = a.step(act)
        ob, tb, db, ib = b.step(act)
        assert torch.equal(a.rows, b.rows) and torch.equal(da, db), calls
        assert sorted(set(ta) - set(tb)) == ['track_cells'] and sorted(set(oa) - set(ob)) == ['track_map']
        assert all(torch.equal(ta[k], tb[k]) for k in tb) and all(torch.equal(ia[k], ib[k]) for k in ia), calls
        assert all(torch.equal(oa[k], ob[k]) for k in ob), calls
        assert ta['track_cells'].data_ptr() == a.env.track_cells.data_ptr()
        a.env.sync()
        for e in range(slots):
            if bool(was_live[e]):
                pose, mu, active, radius = env_tracks(a.env, e)
                want = TM.window(pose, mu, active, radius, a.env.cfg, margin, samples)
                check_window(a.env, want, calls, e)
                nonzero += int(want.any())
            if bool(da[e]) and e not in kept and bool(ia['live'][e]):
                kept[e] = tuple(x.clone() for x in (a.env.track_win[e], oa['track_map'][e], a.env.track_cells[e], a.env.tracks['last_step'][e]))
        info = ia
        calls += 1
    a.close(), b.close()
    assert torch.equal(a.rows, b.rows) and int((a.rows[:, 0] > 0).sum()) == M
    return refills, frozen, nonzero
