"""Synthetic batches for the step path's gaze decision (include/d2d_gaze.h) and what the package's host policies -- gaze.LookAhead and
gaze.Owl, which tests/golden/host_gaze_rows.npz pins to the reference -- answer for them.  test_gaze_host_build.py runs them through
the gcc build of csrc/gaze/d2d_gaze.h, test_gpu_gaze.py through libd2d_gaze.so.  Test infrastructure."""
import functools

import numpy as np

from drone2d_amd import _abi as A

KINDS = ('plain', 'rest', 'on_agent', 'yaw10', 'goal_on_drone', 'late_active', 'axis', 'pm180')
NS = (0, 1, 3, 70, 172)


def params(pkg, **kw):
    return pkg.Params(**dict(dict(planner='Jerk_Primitive', gaze_method='Owl'), **kw))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def batch(B, N, seed=0, cycle='fresh', done_every=0):
    """Inputs of one d2d_gaze_act call over B envs of N trackers.  Env e is of kind KINDS[e % len(KINDS)].
    cycle: 'fresh' (all-zero Owl state: every env decides), 'mixed' (random scores; env e has (e // 3) % 8 calls left, so envs sit at
    different points of their 8-call cycle).  done_every: every that-many-th env (from env 1) has its done flag set."""
    rng = np.random.RandomState(1000 * N + 10 * seed + (cycle == 'mixed'))
    kinds = [KINDS[e % len(KINDS)] for e in range(B)]
    drone = np.zeros((B, A.DF))
    drone[:, A.D_X], drone[:, A.D_Y] = rng.uniform(20, 480, B), rng.uniform(20, 480, B)
    drone[:, A.D_YAW] = rng.uniform(0, 360, B)
    drone[:, A.D_VX], drone[:, A.D_VY] = rng.uniform(-40, 40, B), rng.uniform(-40, 40, B)
    drone[:, A.D_AX:A.D_AY + 1] = rng.uniform(-40, 40, (B, 2))
    target = rng.uniform(0, 500, (B, 2))
    active = (rng.uniform(0, 1, (B, max(N, 1))) < (0.6 if N <= 3 else 0.25)).astype(np.uint8)
    kf = np.zeros((B, max(N, 1), A.KF))
    kf[:, :, 0:2] = rng.uniform(0, 500, (B, max(N, 1), 2))
    kf[:, :, 2:4] = rng.uniform(-20, 20, (B, max(N, 1), 2))
    kf[:, :, 4:] = rng.uniform(0, 1, (B, max(N, 1), 16))
    for e, k in enumerate(kinds):
        if k == 'rest':
            drone[e, A.D_VX:A.D_VY + 1] = 0.0
        elif k == 'on_agent' and N:                    # a tracker exactly on the drone: norm 0 in the weight's denominator
            kf[e, 0, 0:2] = drone[e, A.D_X:A.D_Y + 1]
            active[e, 0] = 1
        elif k == 'yaw10':                             # -yaw % 360 sits on a ten-degree direction
            drone[e, A.D_YAW] = 10.0 * rng.randint(0, 36)
        elif k == 'goal_on_drone':
            target[e] = drone[e, A.D_X:A.D_Y + 1]
        elif k == 'late_active' and N >= 3:            # active trackers after inactive ones: the zip(d_o, trackers) pairing shows
            active[e] = 0
            active[e, N // 2:N] = 1
            active[e, N - 2] = 0
        elif k == 'axis':                              # axis-aligned velocities: atan2 of a signed zero
            v = [(30.0, 0.0), (-30.0, 0.0), (0.0, 30.0), (0.0, -30.0)][(e // len(KINDS)) % 4]
            drone[e, A.D_VX:A.D_VY + 1] = v
        elif k == 'pm180':                             # target_yaw - yaw exactly +180 or -180 (LookAhead's `< 180` rule)
            if (e // len(KINDS)) % 2:
                drone[e, A.D_VX:A.D_VY + 1], drone[e, A.D_YAW] = (-25.0, 0.0), 0.0     # heading 180
            else:
                drone[e, A.D_VX:A.D_VY + 1], drone[e, A.D_YAW] = (25.0, 0.0), 180.0    # heading 0
    if N == 0:
        active[:], kf[:] = 0, 0.0
    owl = np.zeros((B, A.OWL_STATE_F))
    if cycle == 'mixed':
        owl[:, :A.OWL_NDIR] = rng.uniform(0, 1, (B, A.OWL_NDIR))
        owl[:, A.OWL_S_RATE] = rng.choice(np.arange(-80, 80, 8.0), B)
        owl[:, A.OWL_S_LEFT] = (np.arange(B) // 3) % 8
    flags = np.zeros((B, 4), dtype=np.uint8)
    flags[:, :3] = rng.randint(0, 2, (B, 3))
    if done_every:
        flags[1::done_every, A.F_DONE] = 1
    action = rng.uniform(-1, 1, B)                     # what the call must leave in place for a finished env
    return dict(B=B, N=N, kinds=kinds, drone=drone, target=target, active=active[:, :N].copy(), kf=kf[:, :N].copy(), owl_state=owl,
                flags=flags, action=action)


class _Tracker:
    def __init__(self, active, mu):
        self.active = bool(active)
        self.mu_upds = [np.array(mu, dtype=np.float64).reshape(4, 1)]


class _Drone:
    def __init__(self, rec, active, kf):
        self.x, self.y, self.yaw = float(rec[A.D_X]), float(rec[A.D_Y]), float(rec[A.D_YAW])
        self.velocity = np.array([rec[A.D_VX], rec[A.D_VY]], dtype=np.float64)
        self.trackers = [_Tracker(a, m[:4]) for a, m in zip(active, kf)]


def owl_policy(pkg, p, st):
    """a gaze.Owl holding the state of one env's owl_state record"""
    from drone2d_amd import gaze
    o = gaze.Owl(p)
    o.score = np.array(st[:A.OWL_NDIR], dtype=np.float64)
    o.queue = [float(st[A.OWL_S_RATE])] * int(st[A.OWL_S_LEFT])
    return o


def host_answers(pkg, b, kind, p=None, use_flags=True):
    """(action [B], owl_state [B, 40]) after one call of the host policy `kind` for every env of batch `b` that is not done"""
    from drone2d_amd import gaze
    p = params(pkg) if p is None else p
    action, owl = b['action'].copy(), b['owl_state'].copy()
    hold = int(0.8 // p.dt) - 1
    for e in range(b['B']):
        if use_flags and b['flags'][e, A.F_DONE]:
            continue
        obs = dict(drone=_Drone(b['drone'][e], b['active'][e], b['kf'][e]), target=[float(b['target'][e, 0]), float(b['target'][e, 1])])
        if kind == 'LookAhead':
            action[e] = gaze.LookAhead(p).plan(obs)
            continue
        o = owl_policy(pkg, p, owl[e])
        decided = len(o.queue) == 0
        action[e] = o.plan(obs)
        owl[e, :A.OWL_NDIR] = o.score
        assert len(o.queue) == (hold if decided else owl[e, A.OWL_S_LEFT] - 1)
        owl[e, A.OWL_S_LEFT] = len(o.queue)
        if decided:
            owl[e, A.OWL_S_RATE] = action[e] * p.drone_max_yaw_speed if not o.queue else o.queue[0]
    return action, owl


@functools.lru_cache(maxsize=None)
def case(B, N, kind, cycle='fresh', done_every=0, use_flags=True, seed=0):
    """(batch, action, owl_state) with the host policies' answers, computed once per process"""
    import drone2d_amd as pkg
    b = batch(B, N, seed, cycle, done_every)
    a, o = host_answers(pkg, b, kind, use_flags=use_flags)
    return b, a, o


def call_of(pkg, b, kind, ptr, arr, use_flags=True, p=None):
    """the d2d_gaze_call over arrays `arr` (name -> array whose address ptr() gives)"""
    from drone2d_amd import gaze_plugin
    p = params(pkg) if p is None else p
    c = A.GazeCall()
    c.B, c.N, c.kind, c.reserved, c.dt, c.yaw_rate_max = b['B'], b['N'], gaze_plugin.KINDS[kind], 0, p.dt, p.drone_max_yaw_speed
    for k in ('drone', 'target', 'owl_state', 'owl_tab', 'action'):
        setattr(c, k, ptr(arr[k]))
    c.active = ptr(arr['active']) if b['N'] else None
    c.kf = ptr(arr['kf']) if b['N'] else None
    c.flags = ptr(arr['flags']) if use_flags else None
    return c


def owl_tab(pkg, p=None):
    from drone2d_amd import device_plugins
    return device_plugins.owl_table(params(pkg) if p is None else p)
