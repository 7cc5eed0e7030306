"""The recorded rays (tests/golden/scan_episodes.npz, written by tests/golden/make_scan_golden.py) and the comparisons
tests/test_scan_obs_cpu.py (the model backend of tests/scan_backend.py) and tests/test_gpu_scan_obs.py (the HIP library) share.
Every comparison is exact: integers, and the bit patterns of float32 / float64.  Test infrastructure."""
import functools
import json
import os

import numpy as np

import scan_model as SN

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scan_episodes.npz')
EPISODES = 4
NOT_PARAMS = ('seed', 'steps', 'teleport')


@functools.lru_cache(maxsize=None)
def episode(i):
    z = np.load(PATH)
    pre = f'e{i}_'
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    d['cfg'] = json.loads(str(d['cfg']))
    coords, wall, hit = d['coords'], d['wall'], d['hit']
    stopped = ~((coords[..., 0] == -1) & (coords[..., 1] == -1))
    agent = hit.any(axis=-1)
    # the kind of include/d2d_scan.h from the reference's record: an agent stop has wall_hit 0 and a hit list, a wall stop wall 1
    d['kind'] = np.where(~stopped, 0, np.where(agent, 2, np.where(wall == 1, 1, 3))).astype(np.uint8)
    return d


def params_of(pkg, ep, **kw):
    cfg = {k: v for k, v in ep['cfg'].items() if k not in NOT_PARAMS}
    return pkg.Params(**dict(cfg, **kw))


def bits(a):
    """the bit patterns of a float array (or the integers themselves): NaNs and signed zeros compare as what they are"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).sum(axis=-1)


@functools.lru_cache(maxsize=None)
def coverage():
    """what the stored set holds: rays of every kind, agent stops at sample 0 (the ray ends where the drone is), rays holding two or
    more agents, range stops whose raw `wall` is 3, the ray counts and the agent counts"""
    kinds = np.zeros(4, dtype=np.int64)
    sample0 = multi = raw3 = 0
    rays, agents = set(), set()
    for i in range(EPISODES):
        ep = episode(i)
        k = ep['kind']
        kinds += np.bincount(k.reshape(-1), minlength=4)
        at_drone = (ep['coords'][..., 0] == ep['pose'][:, None, 0]) & (ep['coords'][..., 1] == ep['pose'][:, None, 1])
        sample0 += int(((k == 2) & at_drone).sum())
        multi += int((popcount(ep['hit']) >= 2).sum())
        raw3 += int(((k == 3) & (ep['wall'] == 3)).sum())
        rays.add(k.shape[1])
        agents.add(int(ep['cfg']['agent_number']))
    return dict(kinds=tuple(int(v) for v in kinds), sample0=sample0, multi=multi, raw3=raw3, rays=tuple(sorted(rays)),
                agents=tuple(sorted(agents)))


def assert_coverage(cov):
    assert min(cov['kinds']) >= 100 and cov['sample0'] >= 50 and cov['multi'] >= 1 and cov['raw3'] >= 1, cov
    assert 50 in cov['rays'] and 100 in cov['rays'] and min(cov['agents']) <= 32 < max(cov['agents']), cov


def unpack(words, N):
    """[..., words] uint32 -> [..., N] 0 / 1"""
    w = np.ascontiguousarray(words).astype(np.uint32)
    b = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(w.shape[:-1] + (-1,))[..., :N].astype(np.uint8)


def scan_of(env, e=0):
    env.sync()
    return dict(end=env.ray_end[e].cpu().numpy(), kind=env.ray_kind[e].cpu().numpy(), hit=env.scan['hit'][e].cpu().numpy().view(np.uint32),
                obs=env.scan['obs'][e].cpu().numpy(), last_step=int(env.scan['last_step'][e]))


def check_step(env, ep, t, obs=None):
    """env 0 has taken step t of the episode: its rays are the recording's, bit for bit, `wall` through the port's mapping"""
    got = scan_of(env)
    N, R = env.cfg.N, env.cfg.R
    assert got['end'].shape == (R, 2) and np.array_equal(bits(got['end']), bits(ep['coords'][t])), \
        (t, np.argwhere(bits(got['end']) != bits(ep['coords'][t]))[:5].tolist())
    assert np.array_equal(got['kind'], ep['kind'][t]), (t, got['kind'].tolist(), ep['kind'][t].tolist())
    assert np.array_equal(got['hit'], ep['hit'][t]), t
    wall = np.array(SN.WALL_OF_KIND, dtype=np.uint8)[got['kind']]
    raw = ep['wall'][t]
    assert np.array_equal(wall, np.where((ep['kind'][t] == 3) & (raw == 3), 2, raw)), t       # the one deviation: a raw 3 at a range stop
    assert np.array_equal(env.ray_hits[0].cpu().numpy().astype(np.uint8), unpack(ep['hit'][t], N)), t
    obs = env._result()[0] if obs is None else obs
    sc = obs['scan']
    assert tuple(sc.shape) == (1, 2, R) and str(sc.dtype) == 'torch.float32' and sc.data_ptr() == env.scan['obs'].data_ptr()
    sc = sc[0].cpu().numpy()
    assert np.array_equal(sc[1], ep['kind'][t].astype(np.float32)), t
    x0, y0 = ep['pose'][t, 0], ep['pose'][t, 1]
    stopped = ep['kind'][t] != 0
    want = np.sqrt((ep['coords'][t, :, 0] - x0) ** 2 + (ep['coords'][t, :, 1] - y0) ** 2).astype(np.float32)
    assert np.array_equal(bits(sc[0][stopped]), bits(want[stopped])), t
    inside = 0 < x0 < env.cfg.W_px and 0 < y0 < env.cfg.H_px
    assert inside or not sc[0].any(), t                                  # a drone on the map's edge takes no sample: range 0


def step_of(ep):
    """the call that takes one step of the episode's env under the recorded action"""
    def nomove(env, action):
        env.step(action)

    def plugins(env, action):
        env._set_action(action)
        env._plugins_step()
    return nomove if ep['cfg']['planner'] == 'NoMove' else plugins


def env_kw(ep):
    return dict(device_plugins=False, gaze=None) if ep['cfg']['planner'] == 'NoMove' else {}


def replay(env, ep, step=None):
    """the episode's recorded poses and actions through `step(env, action)`, one env: no rays before the first step, then the
    recording's rays after every step.  Returns the steps taken"""
    import torch
    from drone2d_amd import _abi as A
    step = step or step_of(ep)
    T = len(ep['action'])
    first = scan_of(env)
    assert first['last_step'] == 0 and not first['end'].any() and not first['kind'].any() and not first['hit'].any() and not first['obs'].any()
    for t in range(T):
        if not np.isnan(ep['tele'][t, 0]):
            env.state.drone[0, :3] = torch.from_numpy(ep['tele'][t].copy()).to(env.device)
        d = env.state.drone[0].cpu().numpy()
        assert np.array_equal(bits(d[:3]), bits(ep['pose'][t])), (t, d[:3].tolist(), ep['pose'][t].tolist())
        step(env, torch.tensor([float(ep['action'][t])], dtype=torch.float64))
        check_step(env, ep, t)
        assert scan_of(env)['last_step'] == int(env.state.counters[0, A.C_STEPS]) == t + 1
    return T


# ---------------------------------------------------------------------------------------------------------------- handmade poses
POISON = 0xAB
HANDMADE = [     # (map_size, agents, grid layout): 50 x 50, 30 x 20 and 100 x 80 cells, the tiled ones with partial edge tiles
    ([500, 500], 10, 'rowmajor'),
    ([300, 200], 0, 'rowmajor'),
    ([1000, 800], 33, 'tiled'),
    ([500, 500], 72, 'tiled'),
]


def handmade_params(pkg, k):
    size, n, layout = HANDMADE[k]
    return pkg.Params(planner='NoMove', agent_number=n, agent_radius=15, agent_max_speed=20, map_id=3, map_size=list(size),
                      init_pos=[50, 50], target_list=[[size[0] - 50, size[1] - 50]]), layout


def handmade_poses(W_px, H_px):
    """16 envs: (x, y, yaw, steps, last, agents at the drone).  The four corners (inside, one px from the walls), x == 0 and x == W_px
    (no sample), a cell's origin under yaw 0 / 45 / 90 / 135 / 270 (the middle rays' slopes lie at +-1 and 0: both sides of the
    |slope| > 1 branch and both signs of either step), inside an agent, inside two overlapping agents, a finished env (its counter is that of its latest
    update) and an env whose counter is 0: both keep their poison"""
    cx, cy = float(W_px // 20 * 10), float(H_px // 20 * 10)
    P = lambda x, y, yaw, steps=1, last=0, inside=0: dict(x=float(x), y=float(y), yaw=float(yaw), steps=steps, last=last, inside=inside)   # noqa: E731
    return [P(1, 1, 315), P(W_px - 1, 1, 225, 7, 6), P(1, H_px - 1, 45, 2, 0), P(W_px - 1, H_px - 1, 135, 3, 9),
            P(0, cy, 0), P(W_px, cy, 180, 4, 3),
            P(cx, cy, 0), P(cx, cy, 45, 12, 11), P(cx, cy, 90), P(cx, cy, 135, 5, 4), P(cx, cy, 270),
            P(cx + 3.5, cy - 2.25, 33.3, 2, 1, inside=1), P(cx - 40, cy + 30, 200, 6, 2, inside=2),
            P(cx, cy, 10, 5, 5), P(cx, cy, 10, 0, 0), P(W_px - 11.5, H_px - 12.5, 77.7, 9, 0)]


def run_handmade(env, launch, record=None, poses=None, place=None):
    """The poses through `launch()` -- one d2d_scan_update over the env's own structs -- with every buffer the launch may write
    poisoned first, against the model; then a second launch without a step, which must change nothing.  The state and dmap must
    come out as they went in.  `poses`: handmade_poses unless given; `place(agents, walls, poses)`: writes a set's own agents into the
    planes [B, AF, N] and walls into the grids [B, bytes] (the crowd and the ring below).  Returns (envs left alone, rays per kind)"""
    import torch
    from drone2d_amd import _abi as A
    cfg, B = env.cfg, env.num_envs
    poses = handmade_poses(cfg.W_px, cfg.H_px) if poses is None else poses
    assert B == len(poses) == 16
    N, R, hw = cfg.N, cfg.R, env._scan.hit_words
    agents, counters = env.state.agents.cpu().numpy().copy(), env.state.counters.cpu().numpy().copy()
    pose = np.zeros((B, A.DF), dtype=np.float64)
    last = np.zeros(B, dtype=np.int32)
    for e, q in enumerate(poses):
        pose[e, A.D_X], pose[e, A.D_Y], pose[e, A.D_YAW] = q['x'], q['y'], q['yaw']
        counters[e, A.C_STEPS], last[e] = q['steps'], q['last']
        if place is not None:
            continue
        for k in range(min(q['inside'], N)):       # agents whose circle holds the drone: the ray ends at sample 0 with all of them
            agents[e, A.A_PX, k], agents[e, A.A_PY, k] = q['x'] + 4.0 * k - 1.0, q['y'] + 2.0
        if N > 40:                                 # agent 70 in the way of the straight-ahead rays: a bit of the third word
            agents[e, A.A_PX, 70], agents[e, A.A_PY, 70] = q['x'] + 40.0 * np.cos(np.radians(q['yaw'])), q['y'] - 40.0 * np.sin(np.radians(q['yaw']))
    if place is not None:
        walls = env.state.gt.cpu().numpy().reshape(B, -1).copy()
        place(agents, walls, poses)
        env.state.gt.copy_(torch.from_numpy(walls).reshape(env.state.gt.shape).to(env.device))
    poison = lambda shape, dt: np.frombuffer(np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, POISON, dtype=np.uint8).tobytes(), dtype=dt).reshape(shape).copy()   # noqa: E731
    before = dict(end=poison((B, R, 2), np.float64), kind=poison((B, R), np.uint8), hit=poison((B, R, hw), np.int32),
                  obs=poison((B, 2, R), np.float32), last_step=last)
    dev = env.device
    for t, v in ((env.state.agents, agents), (env.state.counters, counters), (env.scan['pose'], pose)) + tuple((env.scan[k], before[k]) for k in before):
        t.copy_(torch.from_numpy(v).to(dev))
    env.state.drone.fill_(float('nan'))            # the launch reads the snapshot, never the drone
    keep = {k: env.state.t[k].clone() for k in ('agents', 'gt', 'dmap', 'counters', 'hit')}
    launch()
    env.sync()
    got = {k: env.scan[k].cpu().numpy() for k in before}
    got['hit'] = got['hit'].view(np.uint32)
    assert all(torch.equal(env.state.t[k], keep[k]) for k in keep)
    gt = env.state.gt.cpu().numpy().reshape(B, -1)
    alone, kinds = 0, np.zeros(4, dtype=np.int64)
    for e, q in enumerate(poses):
        out = SN.update(last[e], q['steps'], pose[e], agents[e], gt[e], cfg, hw)
        if out is None:
            for k in before:
                assert np.array_equal(bits(got[k][e]), bits(before[k][e].view(got[k].dtype) if k == 'hit' else before[k][e])), (e, k)
            alone += 1
            continue
        end, kind, hit, obs = out
        assert np.array_equal(got['kind'][e], kind), (e, got['kind'][e].tolist(), kind.tolist())
        assert np.array_equal(bits(got['end'][e]), bits(end)), (e, np.argwhere(bits(got['end'][e]) != bits(end))[:5].tolist())
        assert np.array_equal(got['hit'][e], hit), e
        assert np.array_equal(bits(got['obs'][e]), bits(obs)), (e, np.argwhere(bits(got['obs'][e]) != bits(obs))[:5].tolist())
        assert got['last_step'][e] == q['steps'], e
        if q['inside'] and N >= q['inside']:
            assert (kind == 2).all() and (popcount(hit) >= q['inside']).all(), e
        if not (0 < q['x'] < cfg.W_px):
            assert not kind.any() and (end == -1).all() and not obs.any(), e
        kinds += np.bincount(kind, minlength=4)
    launch()
    env.sync()
    for k in before:
        now = env.scan[k].cpu().numpy()
        assert np.array_equal(bits(now.view(np.uint32) if k == 'hit' else now), bits(got[k])), k
    if record is not None:
        record.append(dict(cfg=cfg, hit_words=hw, agents=agents, counters=counters, gt=gt, pose=pose, before=before, want=got))
    return alone, tuple(int(v) for v in kinds)


# ---------------------------------------------------------------------------------------------------------------- the crowd, the ring
CCAP = 64                            # D2D_SCAN_CCAP of csrc/scan/d2d_scan.h: an env with more candidates tests every agent
CROWD_COUNTS = (63, 64, 65, 72)      # candidates of env e: CROWD_COUNTS[e % 4] -- below, at and above the list's capacity, and everyone
CROWD_N = 72                         # three hit words
CROWD_R2 = 2.5 ** 2                  # small circles: a ray of such a crowd can pass between them (radius 15 stops every ray in an agent)
RING_N = 33                          # d = 0, 0.5 .. 16 px beyond radius + depth
RING_RADIUS = 5.0


def near(px, py, r2, x0, y0, depth, ss):
    """the documented cull bound of d2d_scan_near (csrc/scan/d2d_scan.h), restated: may this agent hold a sample of the drone's rays?"""
    lim = np.sqrt(r2) + depth + 1.5 * ss + 2.0
    dx, dy = px - x0, py - y0
    return dx * dx + dy * dy <= lim * lim


def candidates(cfg, pose, agents):
    """[B] the candidates of every env under `near`, [B, N] which they are"""
    from drone2d_amd import _abi as A
    ss = float(cfg.scale) - 1.0
    is_near = near(agents[:, A.A_PX], agents[:, A.A_PY], agents[:, A.A_R2], pose[:, A.D_X, None], pose[:, A.D_Y, None], float(cfg.depth), ss)
    return is_near.sum(axis=1), is_near


def crowd_params(pkg):
    return pkg.Params(planner='NoMove', agent_number=CROWD_N, agent_radius=15, agent_max_speed=20, map_id=3, map_size=[500, 500],
                      init_pos=[50, 50], target_list=[[450, 450]]), 'tiled'


def ring_params(pkg):
    return pkg.Params(planner='NoMove', agent_number=RING_N, agent_radius=15, agent_max_speed=20, map_id=3, map_size=[500, 500],
                      init_pos=[50, 50], target_list=[[450, 450]]), 'rowmajor'


CROWD_AT = (260.0, 240.0)            # a cell's origin near the centre
CROWD_WALLS = ((5, 0), (-5, 0), (0, 5), (0, -5), (4, 4), (-4, 4), (4, -4), (-4, -4))      # cells from the drone's: within the range


def crowd_poses(W_px, H_px):
    """16 envs at one cell's origin near the centre, yaw 22.5 * e: the four envs of a candidate count (e % 4) look into all four
    quadrants"""
    return [dict(x=CROWD_AT[0], y=CROWD_AT[1], yaw=22.5 * e, steps=1 + e % 3, last=0, inside=0) for e in range(16)]


def crowd_place(cfg):
    """place(agents, walls, poses) of the crowd: env e has CROWD_COUNTS[e % 4] agents scattered within the range of its drone -- three
    of them laid over three others, so that a sample lies in two -- and the rest parked in the far corner.  The parked ones have
    indices below 64 (another choice in every env), so agents 64 .. 71 are candidates everywhere: the second pass of the device's
    cull always adds to the list, up to slot 63 exactly in the envs of 64 candidates and past it in those of 65.  Map 3 has walls on
    its border alone, farther from the centre than the range: eight OCCUPIED cells go around the drone, with gaps between them"""
    from drone2d_amd import _abi as A
    depth = float(cfg.depth)

    def place(agents, walls, poses):
        rs = np.random.RandomState(72)
        N = agents.shape[2]
        assert N == CROWD_N
        for e, q in enumerate(poses):
            parked = sorted({(3 * e + 5 * j) % 64 for j in range(N - CROWD_COUNTS[e % 4])})
            assert len(parked) == N - CROWD_COUNTS[e % 4]
            rho, phi = depth * np.sqrt(rs.uniform(0.01, 1.0, N)), rs.uniform(0, 2 * np.pi, N)
            agents[e, A.A_PX], agents[e, A.A_PY] = q['x'] + rho * np.cos(phi), q['y'] + rho * np.sin(phi)
            for k in (64, 66, 68):                 # pairs a sample can lie in together: bits of the third word with a neighbour's
                agents[e, A.A_PX, k + 1], agents[e, A.A_PY, k + 1] = agents[e, A.A_PX, k] + 1.0, agents[e, A.A_PY, k] - 0.5
            agents[e, A.A_R2] = CROWD_R2
            for j, k in enumerate(parked):
                agents[e, A.A_PX, k], agents[e, A.A_PY, k] = 3.0 + 2.0 * (j % 4), 3.0 + 2.0 * (j // 4)
            ci, cj = int(q['x'] // cfg.scale), int(q['y'] // cfg.scale)
            for di, dj in CROWD_WALLS:
                walls[e, SN.grid_index(ci + di, cj + dj, cfg.H, cfg.grid_tile)] = A.OCCUPIED
    return place


def check_crowd(cfg, rec):
    """the record run_handmade left of the crowd is what the set is for: the candidate counts under the documented bound (a later
    change of the bound fails here, it does not turn the case back into the small-list path), agents 64 .. 71 among the candidates of
    every env, and by the model alone rays of every kind a drone inside the map can have -- stopped by a wall, by an agent and by the
    range (kind 0 is a ray that leaves the map: with the range at 80 px none of a drone at the centre does) -- in every group, some
    of them inside two agents at once"""
    count, is_near = candidates(cfg, rec['pose'], rec['agents'])
    assert count.tolist() == [CROWD_COUNTS[e % 4] for e in range(16)], count.tolist()
    assert is_near[:, 64:].all()
    kind, hit = rec['want']['kind'], rec['want']['hit']
    for g in range(4):
        kinds = np.bincount(kind[g::4].reshape(-1), minlength=4)
        assert kinds[0] == 0 and kinds[1] >= 1 and kinds[2] >= 1 and kinds[3] >= 1, (g, kinds.tolist())
        assert int((popcount(hit[g::4]) >= 2).sum()) >= 1, g
        assert hit[g::4, :, 2].any(), g            # an agent of index >= 64 was met


def ring_poses(W_px, H_px):
    """16 envs at the centre cell's origin, yaws 0, 7.3 .. 109.5: the step of a ray is 9 .. 12.7 px long, so its last sample lies
    0 .. 12.7 px beyond the range"""
    return [dict(x=250.0, y=250.0, yaw=7.3 * e, steps=1, last=0, inside=0) for e in range(16)]


def ring_place(cfg):
    """place(agents, walls, poses) of the ring: agent k of env e is centred on ray (7 k + 3 e) % R at distance radius + depth + k / 2 from the
    drone, k = 0 .. 32.  The last sample of a ray lies up to a step beyond the range, so a circle whose rim is that far out holds a
    genuine sample; a cull bound that is too tight drops it, one that is right keeps every agent the model's loop over all agents meets"""
    from drone2d_amd import _abi as A

    def place(agents, walls, poses):
        N = agents.shape[2]
        assert N == RING_N
        for e, q in enumerate(poses):
            for k in range(N):
                i = (7 * k + 3 * e) % cfg.R
                ang = SN.positive_angle((np.pi * 2 - q['yaw'] * (np.pi / 180)) + float(cfg.ray_off0) + float(cfg.ray_dth) * i)
                dist = RING_RADIUS + float(cfg.depth) + 0.5 * k
                agents[e, A.A_PX, k], agents[e, A.A_PY, k] = q['x'] + dist * np.cos(ang), q['y'] + dist * np.sin(ang)
            agents[e, A.A_R2] = RING_RADIUS ** 2
    return place


def check_ring(cfg, rec):
    """the ring is at the bound: agents on either side of it, and by the model alone hits of agents whose rim is more than half a
    step (+ 2 px) beyond the range -- the ones a bound of depth + 0.5 * (scale - 1) + 2 would have dropped"""
    count, is_near = candidates(cfg, rec['pose'], rec['agents'])
    assert 0 < count.min() and count.max() < RING_N and (count <= CCAP).all(), count.tolist()
    met = unpack(np.bitwise_or.reduce(rec['want']['hit'], axis=1), RING_N)            # [B, N]: the agents some ray of the env met
    beyond = 0.5 * np.arange(RING_N)
    ss = float(cfg.scale) - 1.0
    assert int(met[:, beyond > 0.5 * ss + 2.0].sum()) >= 8, met.sum(axis=0).tolist()
    assert not met[~is_near].any()                 # the documented bound itself drops nobody the model meets
    return int(met.sum())


SPECIAL = {'crowd': (crowd_params, crowd_poses, crowd_place, check_crowd), 'ring': (ring_params, ring_poses, ring_place, check_ring)}


def run_special(env, name, launch, record=None):
    """the crowd or the ring through run_handmade, then the set's own coverage check on the record"""
    _, poses, place, check = SPECIAL[name]
    rec = []
    out = run_handmade(env, launch, rec, poses=poses(env.cfg.W_px, env.cfg.H_px), place=place(env.cfg))
    check(env.cfg, rec[0])
    if record is not None:
        record.extend(rec)
    return out


def check_cleared(env, e):
    """slot e shows no rays: what a fresh world, a reset and a refill leave"""
    got = scan_of(env, e)
    assert got['last_step'] == 0 and not got['end'].any() and not got['kind'].any() and not got['hit'].any() and not got['obs'].any(), e


def check_against_model(env, e):
    """slot e's rays are the model's for the snapshot pose and the agents as they stand"""
    got = scan_of(env, e)
    gt = env.state.gt[e].cpu().numpy().reshape(-1)
    end, kind, hit, obs = SN.scan(env.scan['pose'][e].cpu().numpy(), env.state.agents[e].cpu().numpy(), gt, env.cfg, env._scan.hit_words)
    assert np.array_equal(got['kind'], kind) and np.array_equal(bits(got['end']), bits(end)) and np.array_equal(got['hit'], hit), e
    assert np.array_equal(bits(got['obs']), bits(obs)), e
    return kind


def stream_pair(make, p, slots, M, refill_every=4, limit=2000):
    """The stream with the channel against the stream without it, turn for turn and step for step: rows, terms, done, local_map and
    yaw_angle are equal; every refilled slot shows the cleared channel at its step 0; a slot that has stepped shows the model's rays
    with its own step counter; a finished slot keeps its rays until the turn.  make(p, slots, scan_obs) -> env.  Returns (refills,
    frozen slot-steps checked)"""
    import torch
    from action_stream_backend import policy
    a = make(p, slots, True).action_stream(M, refill_every=refill_every)
    b = make(p, slots, False).action_stream(M, refill_every=refill_every)
    assert a.env.scan is not None and b.env.scan is None
    for e in range(slots):
        check_cleared(a.env, e)
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
                check_cleared(a.env, e)
                kept.pop(e, None)
                refills += 1
            elif e in kept:                                                                  # done, not yet refilled: as it ended
                assert bool(done[e])
                now = (a.env.ray_end[e], a.env.ray_kind[e], a.env.scan['hit'][e], obs['scan'][e], a.env.scan['last_step'][e])
                assert all(torch.equal(x, y) for x, y in zip(now, kept[e])), e
                frozen += 1
        act = policy(info['episode'], info['steps'])
        oa, ta, da, ia = a.step(act)
        ob, tb, db, ib = b.step(act)
        assert torch.equal(a.rows, b.rows) and torch.equal(da, db), calls
        assert sorted(set(oa) - set(ob)) == ['scan'] and set(ta) == set(tb)
        assert all(torch.equal(ta[k], tb[k]) for k in tb) and all(torch.equal(ia[k], ib[k]) for k in ia), calls
        assert torch.equal(oa['local_map'], ob['local_map']) and torch.equal(oa['yaw_angle'], ob['yaw_angle']), calls
        a.env.sync()
        for e in range(slots):
            if bool(ia['live'][e]):
                assert int(a.env.scan['last_step'][e]) == int(ia['steps'][e]) >= 1, (calls, e)
                if calls % 5 == e % 5:             # (the model is plain Python: a fifth of the slot-steps)
                    check_against_model(a.env, e)
            if bool(da[e]) and e not in kept and bool(ia['live'][e]):
                kept[e] = tuple(x.clone() for x in (a.env.ray_end[e], a.env.ray_kind[e], a.env.scan['hit'][e], oa['scan'][e], a.env.scan['last_step'][e]))
        info = ia
        calls += 1
    a.close(), b.close()
    assert torch.equal(a.rows, b.rows) and int((a.rows[:, 0] > 0).sum()) == M
    return refills, frozen
