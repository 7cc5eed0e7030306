"""yaw_planner.Owl (reference lines 151-222) as a BLAS-free scalar model: Python floats, libm `fma` / `pow` through ctypes.

Test infrastructure, like replay.py and oracle_lib.py.  numpy's two-element `dot` / `norm` and the five-element `dot` of the
reference are restated as the FMA chains this host's BLAS performs (test_owl_gaze_cpu.py checks the model against the package's
host policy `gaze.Owl`, i.e. against numpy, on every decision of the golden Owl episodes); the GPU tests compare the device
stage with this model and with the committed fixtures, never with numpy's `dot` on the GPU machine, which may dispatch another
BLAS kernel.  The model is also the specification of the device stage `owl_gaze_env` (csrc/d2d_plugins.h): same operations, same
order, same state (36 scores, the held rate, the calls left that repeat it).
"""
import ctypes
import math

import numpy as np

_libm = ctypes.CDLL('libm.so.6')
for _n, _k in (('fma', 3), ('pow', 2)):
    getattr(_libm, _n).restype = ctypes.c_double
    getattr(_libm, _n).argtypes = [ctypes.c_double] * _k
fma, cpow = _libm.fma, _libm.pow
nan = math.nan

NRATE, NDIR = 20, 36
HOLD_DT = 0.8                                   # Owl.dt
WEIGHTS = (0.2, 0.9, 1.0, 0.1, 0.0)             # Owl.lamb


def div(a, b):
    """IEEE-754 a / b (numpy's float64 division: no ZeroDivisionError)"""
    if b != 0 or b != b or a != a:
        return a / b
    if a == 0:
        return nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def mod360(a):
    return nan if a != a else a % 360.0


def apart(a, b):
    """angle_between (:144-149); np.minimum hands a NaN on"""
    d = abs(mod360(a) - mod360(b))
    if d != d:
        return nan
    e = 360 - d
    return d if d < e else e


def norm2(a, b):
    """numpy.linalg.norm of [a, b]: sqrt of the two-element dot"""
    return math.sqrt(fma(b, b, a * a))


def hold_calls(dt):
    """The calls that repeat a decision (:220), with the reference's Python expression"""
    return int(HOLD_DT // dt) - 1


class OwlModel:
    """One policy object: `plan(...)` is Owl.plan on explicit inputs.  `trackers`: [(active, (mx, my, mvx, mvy)), ...] in tracker
    order, the state of EVERY tracker whatever its active bit (what `tracker.mu_upds[-1]` holds)."""

    def __init__(self, top, fov, depth, dt):
        self.top = float(top)
        self.rates = [float(v) for v in np.arange(-top, top, top / 10)]                 # :161
        assert len(self.rates) == NRATE
        self.fov, self.depth = float(fov), float(depth)
        self.hold = hold_calls(dt)
        self.dirs = [(math.cos(math.radians(d)), math.sin(math.radians(d))) for d in range(0, 360, 10)]
        self.score = [0.0] * NDIR
        self.rate, self.left = 0.0, 0               # the held rate and len(Owl.u)
        self.costs = None                           # of the latest decision

    @classmethod
    def from_params(cls, p):
        return cls(p.drone_max_yaw_speed, p.drone_view_range, p.drone_view_depth, p.dt)

    def state(self):
        """The env's record of d2d_plan.owl_state"""
        return np.array(self.score + [self.rate, float(self.left), 0.0, 0.0], dtype=np.float64)

    def unseen(self, th):
        """G (:169-173)"""
        if apart(th, 0.0) <= self.fov / 2:
            return 0.0
        return math.radians(apart(th, self.fov / 2)) * math.radians(apart(th, -self.fov / 2))

    def lookup(self, th):
        """U (:183-185): np.argmin answers the first minimum, and the first NaN outright"""
        best, bi = None, 0
        for k in range(NDIR):
            a = apart(10.0 * k, th)
            if a != a:
                return self.score[k]
            if best is None or a < best:
                best, bi = a, k
        return self.score[bi]

    def refresh(self, yaw, vx, vy):
        """update_U (:175-181)"""
        mx, my = vx * HOLD_DT, vy * HOLD_DT
        for k in range(NDIR):
            c, sn = self.dirs[k]
            g = -fma(my, sn, mx * c) / self.depth
            g += 0.4 if apart(10.0 * k, -yaw) < self.fov / 2 else -0.05
            self.score[k] = float(max(min(self.score[k] + g, 1), 0))     # U_list is a float64 array

    def decide(self, x, y, yaw, vx, vy, tx, ty, trackers):
        """One decision (:198-218): refreshes the scores, returns the 20 costs"""
        self.refresh(yaw, vx, vy)
        deg = math.degrees
        d_g = deg(math.atan2(ty - y, tx - x))
        n = norm2(vx, vy)
        d_v = deg(math.atan2(div(vy, n), div(vx, n)))
        d_o = [deg(math.atan2(m[1] - y, m[0] - x)) for a, m in trackers if a]
        pull = []
        for j in range(len(d_o)):               # zip(d_o, trackers): the j-th entry takes its weight from tracker j
            m = trackers[j][1]
            pull.append(div(1 * norm2(m[2], m[3]), norm2(m[0] - x, m[1] - y)))
        goal_unknown, flight_unknown = 1 - self.lookup(d_g), 1 - self.lookup(d_v)
        speed2 = cpow(norm2(vx / 10, vy / 10), 2.0)
        costs = []
        for r in self.rates:
            h = -(yaw + r * HOLD_DT)
            t0 = self.unseen(h - d_g) * goal_unknown
            t1 = speed2 * self.unseen(h - d_v) * flight_unknown
            t2 = 0.0
            for w, d in zip(pull, d_o):
                t2 += w * self.unseen(h - d)
            t3 = self.lookup(h)
            t4 = abs(math.radians(r * HOLD_DT))
            acc = 0.0
            for t, l in zip((t0, t1, t2, t3, t4), WEIGHTS):
                acc = fma(t, l, acc)
            costs.append(acc)
        self.costs = costs
        return costs

    @staticmethod
    def argmin(costs):
        for i, c in enumerate(costs):
            if c != c:
                return i
        return min(range(len(costs)), key=lambda i: costs[i])

    def plan(self, x, y, yaw, vx, vy, tx, ty, trackers):
        """Owl.plan (:187-222): the action; `self.decided` says whether this call decided"""
        if self.left > 0:
            self.left -= 1
            self.decided = False
            return self.rate / self.top
        self.decided = True
        self.rate = self.rates[self.argmin(self.decide(x, y, yaw, vx, vy, tx, ty, trackers))]
        self.left = self.hold
        return self.rate / self.top


def inputs_of(state, e):
    """plan()'s arguments for env e from a BatchState on the host (numpy views of drone, target, active, kf)"""
    from drone2d_amd import _abi as A
    d = state['drone'][e]
    trk = [(bool(state['active'][e, j]), [float(v) for v in state['kf'][e, j, :4]]) for j in range(state['active'].shape[1])]
    return (float(d[A.D_X]), float(d[A.D_Y]), float(d[A.D_YAW]), float(d[A.D_VX]), float(d[A.D_VY]),
            float(state['target'][e, 0]), float(state['target'][e, 1]), trk)


def host_state(env):
    """The arrays inputs_of() reads, pulled from a VecDrone2DEnv once"""
    s = env.state
    return {k: getattr(s, k).cpu().numpy() for k in ('drone', 'target', 'active', 'kf')}
