"""The recorded draw calls (tests/golden/render_calls.npz, written by tests/golden/make_render_golden.py), the handmade display lists,
and what tests/test_render_model_cpu.py, tests/test_render_host_build.py and tests/test_gpu_render.py share.  Test infrastructure."""
import functools
import json
import os

import numpy as np

import render_model as RM

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'render_calls.npz')
EPISODES = 4
ITEM_BYTES = 176
NGEOM = {RM.DISC: 3, RM.LINE: 4, RM.ARC: 6}           # the numbers the reference passes per call (POLY: 2 per point)
COLOUR_INDEX = np.array([2, 0, 1, 1], dtype=np.uint8)   # grid code -> the fixture's colour index (240, 100, 200, 200)


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


def frame_calls(ep, f):
    """[(kind, rgb, width, npts, numbers)] of recorded frame f"""
    out = []
    for n in range(int(ep['item_start'][f]), int(ep['item_start'][f + 1])):
        g = ep['geom'][int(ep['geom_start'][n]):int(ep['geom_start'][n + 1])]
        out.append((int(ep['kind'][n]), tuple(int(v) for v in ep['rgb'][n]), float(ep['width'][n]), int(ep['npts'][n]), g))
    return out


def assert_list_is(lst, calls, where=''):
    """the display list (arrays, one slot) equals the reference's calls: count, kinds, colours, widths and every number, as bits"""
    assert int(lst['count']) == len(calls), (where, int(lst['count']), len(calls))
    for n, (kind, rgb, width, npts, g) in enumerate(calls):
        assert int(lst['kind'][n]) == kind and tuple(int(v) for v in lst['rgb'][n]) == rgb, (where, n, kind, int(lst['kind'][n]))
        assert float(lst['width'][n]) == width and int(lst['npts'][n]) == npts, (where, n, kind)
        got = np.ascontiguousarray(np.asarray(lst['geom'][n], dtype=np.float64)[:len(g)])
        assert len(g) == (2 * npts if kind == RM.POLY else NGEOM[kind]), (where, n)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(g).view(np.uint64)), (where, n, kind, got.tolist(), g.tolist())


@functools.lru_cache(maxsize=None)
def coverage():
    """(frames, frames with an active and an inactive tracker together, frames with a polyline, frames without, frames with pillars)"""
    frames = both = withline = without = pillars = 0
    for i in range(EPISODES):
        ep = episode(i)
        for f in range(len(ep['frame_step'])):
            calls = frame_calls(ep, f)
            cols = {c[1] for c in calls if c[0] == RM.DISC}
            frames += 1
            both += int((130, 176, 210) in cols and (200, 36, 35) in cols)
            line = any(c[0] == RM.LINE and c[1] == (0, 0, 0) for c in calls)
            withline += int(line)
            without += int(not line)
            pillars += int((130, 130, 130) in cols)
    return frames, both, withline, without, pillars


def assert_coverage(cov):
    frames, both, withline, without, pillars = cov
    assert frames >= 16 and both >= 1 and withline >= 1 and without >= 1 and pillars >= 1, cov


# ---------------------------------------------------------------------------------------------------------------- an env's state
def slot_state(env, e):
    """what the model's make_list takes, from slot e of a VecDrone2DEnv as it stands (host copies)"""
    s, N = env.state, env.cfg.N
    traj = None
    if env.plugins is not None and 'traj' in env.plugins.t and env.plugins.planner == 1:
        head, stored = (int(v) for v in env.plugins.t['traj_hdr'][e].cpu())
        traj = env.plugins.t['traj'][e, head:stored, :2].cpu().numpy()
    return dict(drone=s.drone[e].cpu().numpy(), agents=s.agents[e].cpu().numpy().reshape(6, N), active=s.active[e].cpu().numpy(),
                vel=s.agent_vel[e].cpu().numpy() if env.rvo and N else None, target=s.target[e].cpu().numpy(),
                pillars=s.pillars[e].cpu().numpy(), traj=traj, R=float(env.cfg.depth), view_range=float(env.params.drone_view_range),
                drone_radius=float(env.cfg.drone_radius), steps=int(s.counters[e, 0]), n_seeded=min(int(env.params.agent_number), N))


def model_list(env, e, traj=None):
    st = slot_state(env, e)
    if traj is not None:
        st['traj'] = traj
    return RM.make_list(**st)


def oracle_env(pkg, ep):
    """(a one-slot env of the episode's world on the CPU oracle backends, step(action))"""
    import torch
    import tracks_backend as TB
    from drone2d_amd import vec_env
    from oracle_lib import OracleBackend
    p = params_of(pkg, ep)
    if p.planner == 'NoMove':
        env = vec_env.VecDrone2DEnv(p, 1, device='cpu', backend=OracleBackend())
        return env, lambda a: env.step(np.array([a]))
    env = TB.env_of(p, 1, **(dict(jerk_tie=tie_table()) if p.planner == 'Jerk_Primitive' else {}))

    def step(a):
        env._set_action(torch.tensor([a], dtype=torch.float64))
        env._jerk_step(True) if env.jerk is not None else env._plugins_step()
    return env, step


def straight_planner():
    """a host planner plugin with the reference's interface, registered as 'Straight': it keeps twelve waypoints on the straight
    line from the drone to its target, 4 px apart, so that the facade has a stored trajectory on the host to upload"""
    from drone2d_amd import planners

    class Straight(planners.Planner):
        def replan_check(self, drone):
            return False, None

        def plan(self, drone, update_t):
            start, goal = np.array([drone.x, drone.y], dtype=np.float64), np.asarray(self.target[:2], dtype=np.float64)
            step = (goal - start) / max(np.linalg.norm(goal - start), 1e-9) * 4.0
            self.trajectory.clear()
            for k in range(1, 13):
                self.trajectory.positions.append(start + k * step)
                self.trajectory.velocities.append(step / update_t)
                self.trajectory.accelerations.append(np.zeros(2))
            return True
    planners.register_planner('Straight', Straight)
    return 'Straight'


def dmap_of(env, e):
    """[W, H] grid codes of slot e's explored map, whatever the device layout"""
    return env.state.logical('dmap')[e].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- handmade lists
def to_bytes(lst, cap):
    """the list as cap packed d2d_render_item records (uint8 [cap, 176]), the rows from count on poisoned"""
    n = int(lst['count'])
    assert n <= cap
    raw = np.full((cap, ITEM_BYTES), 0xAB, dtype=np.uint8)
    raw[:n, 0:4] = lst['kind'].astype(np.int32).reshape(n, 1).view(np.uint8)
    raw[:n, 4:7] = lst['rgb']
    raw[:n, 7] = lst['npts']
    raw[:n, 8:16] = lst['width'].astype(np.float64).reshape(n, 1).view(np.uint8)
    raw[:n, 16:] = lst['geom'].astype(np.float64).reshape(n, 20).view(np.uint8)
    return raw


def digest(a):
    """FNV-1a, 64 bit, over the array's bytes"""
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def _cells(rs, W, H):
    return rs.randint(0, 4, size=(W, H)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def handmade():
    """[dict(name, W_px, H_px, scale, d, W, H, cells [W, H], list)]: the shapes an episode never produces.  The frame of 200 x 130 px
    is ragged against the 128 x 32 pixel tile and against the 16-pixel run; 203 px make a row pitch of 609 bytes, no multiple of 16,
    and a last column of cells only 3 px wide; with W = 20 cells for 203 px the last pixels lie beyond the map"""
    rs = np.random.RandomState(5)
    col = lambda: tuple(int(v) for v in rs.randint(0, 256, 3))       # noqa: E731
    corners = [RM.disc(col(), 0, 0, 6), RM.disc(col(), 199, 129, 6), RM.disc(col(), 199, 0, 4.5), RM.disc(col(), 0, 129, 4.5),
               RM.line(col(), 120, 28, 136, 36, 3), RM.line(col(), 0, 64, 199, 64.5, 2), RM.line(col(), 127.5, 0, 128.5, 129, 1),
               RM.poly(col(), [(100, 20), (150, 30), (160, 70), (128, 50), (90, 75)]), RM.line(col(), 50, 50, 50, 50, 9),
               RM.disc(col(), 128, 32, 0.0), RM.poly(col(), [(10, 100), (40, 100), (40, 125), (10, 125)]),
               RM.poly(col(), [(170, 100), (190, 120)]), RM.line(col(), 180, 10, 140, 10, 0)]
    nan = float('nan')
    outside = [RM.disc(col(), -50, -50, 10), RM.line(col(), 400, 10, 500, 90, 4), RM.disc(col(), nan, 50, 10), RM.line(col(), 10, nan, 60, 60, 2),
               RM.poly(col(), [(-30, -5), (-5, -30), (-40, -40)]), RM.arc(col(), 600, 600, 40, 30, 90), RM.disc(col(), 100, 200, 20),
               RM.disc(col(), 100, 60, 12), RM.disc(col(), 210, 60, 12), RM.line(col(), -20, 100, 30, 110, 6), RM.disc(col(), 1e300, 1e300, 1e300),
               (7, col(), 1.0, 0, np.zeros(20))]
    many = []
    for n in range(300):
        x, y = rs.uniform(-10, 210), rs.uniform(-10, 140)
        if n % 3 == 0:
            many.append(RM.disc(col(), x, y, rs.uniform(1, 25)))
        elif n % 3 == 1:
            many.append(RM.line(col(), x, y, x + rs.uniform(-60, 60), y + rs.uniform(-60, 60), float(rs.randint(1, 6))))
        else:
            many.append(RM.poly(col(), [(x + rs.uniform(-20, 20), y + rs.uniform(-20, 20)) for _ in range(int(rs.randint(3, 11)))]))
    arcs = [RM.arc(col(), 40, 40, 30, 0, 90), RM.arc(col(), 110, 40, 30, 33, 120, 5), RM.arc(col(), 170, 45, 28, 270, 180),
            RM.arc(col(), 50, 100, 28, 201.5, 270, 3), RM.arc(col(), 120, 100, 25, 77, 360), RM.arc(col(), 175, 100, 20, 45, 400, 30),
            RM.arc(col(), 100, 65, 60, -90, 90, 1)]
    out = []

    def case(name, items, W_px=200, H_px=130, scale=10, d=1, W=None):
        W = -(-W_px // scale) if W is None else W
        H = -(-H_px // scale)
        out.append(dict(name=name, W_px=W_px, H_px=H_px, scale=scale, d=d, W=W, H=H, cells=_cells(rs, W, H), list=RM.pack(items)))
    case('corners', corners)
    case('outside', outside)
    case('many', many)
    case('arcs', arcs)
    for d in (2, 3):
        case(f'many-d{d}', many, d=d)
        case(f'arcs-d{d}', arcs, d=d)
        case(f'corners-d{d}', corners, d=d)
    case('pitch-203', corners + arcs, W_px=203)
    case('pitch-203-d3', many, W_px=203, d=3)
    case('beyond-the-map', corners, W_px=203, H_px=133, W=20)
    case('scale-7-d2', arcs + corners, W_px=200, H_px=130, scale=7, d=2)
    case('empty', [])
    case('one-row', many, W_px=640, H_px=1)
    return out


def model_frame(c):
    return RM.raster(c['list'], c['cells'], c['W_px'], c['H_px'], c['scale'], c['d'])
