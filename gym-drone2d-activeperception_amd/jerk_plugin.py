"""Host side of the Jerk_Primitive planner on the device (include/d2d_jerk.h): the tables the library takes as inputs, and the
per-batch state it works on.

Everything of a primitive that depends only on (heading, drone_max_speed, dt) -- the end point offset, the duration and its
powers, the sample times and their powers (traj_planner.py:415-440) -- is evaluated HERE, with numpy's own cos / sin / scalar `**`
of the running host, and handed to the device as `th_tab` / `tt_tab`: the device then runs no pow, cos or sin.

The tie table.  The reference ranks the 72 headings with `cost[:, 0].argsort()`, numpy's default sort, which is not stable: for a
goal on a heading (35 tied pairs) or exactly midway between two (36 tied pairs) the order inside a pair depends on the numpy build
and on the CPU it dispatches for.  A comparison sort's answer depends only on the weak order of its keys, and there are 72 x 4 weak
orders: goal bin k x {phi on theta_k, lower half of the bin, exactly midway, upper half}.  `tie_table()` records the running host's
`np.argsort` for one representative phi of each, checks it on other phi of the same pattern and on a monotone re-labelling of the
keys, and raises if numpy does not answer consistently.  The device ranks by (cost, index) and takes a table row where the row's
weak order is that of the costs at hand; see include/d2d_jerk.h.
"""
import math

import numpy as np

from . import _abi as A

THETAS = np.arange(0, 360, 5)
END_DISTANCE = 30                      # Jerk_Primitive.d
_REPRESENTATIVE = (0.0, 1.0, 2.5, 4.0)  # offset of phi inside a 5-degree bin, per pattern kind
_OTHERS = ((), (0.5, 1.75, 2.25), (), (2.75, 3.5, 4.5))


def heading_costs(phi_h):
    """cost of every heading for the goal direction phi_h (degrees), traj_planner.py:476-479: squared angular distance"""
    goal = phi_h % 360
    out = np.zeros(len(THETAS))
    for i, theta in enumerate(THETAS):
        apart = abs(theta % 360 - goal)
        if not apart <= 180:
            apart = 360 - apart
        out[i] = apart ** 2
    return out


def pattern_of(phi_h):
    """4 * bin + kind of the goal direction: d2d_jerk_pattern of csrc/jerk/d2d_jerk.h, operation for operation"""
    pm = phi_h % 360
    if not 0.0 <= pm < 360.0:
        return 0
    k = int(math.floor(pm / 5.0))
    r = pm - 5.0 * k
    kind = 0 if r == 0.0 else 1 if r < 2.5 else 2 if r == 2.5 else 3
    return 4 * min(k, A.JERK_NTHETA - 1) + kind


def table_fits(perm, eq, cost):
    """does (perm, eq), one row of the tie table, describe the weak order of `cost`?  (d2d_jerk_table_fits)"""
    perm = np.asarray(perm, dtype=np.int64)
    if sorted(perm.tolist()) != list(range(A.JERK_NTHETA)):
        return False
    a, b = cost[perm[:-1]], cost[perm[1:]]
    return bool(np.all(np.where(np.asarray(eq[:-1], dtype=bool), a == b, a < b)))


def tie_table(argsort=np.argsort):
    """(tie_perm, tie_eq) uint8 [288, 72] of the running host's `argsort`; RuntimeError if it is not a function of the weak order"""
    perm = np.zeros((A.JERK_PATTERNS, A.JERK_NTHETA), dtype=np.uint8)
    eq = np.zeros((A.JERK_PATTERNS, A.JERK_NTHETA), dtype=np.uint8)
    for pat in range(A.JERK_PATTERNS):
        k, kind = divmod(pat, 4)
        cost = heading_costs(5.0 * k + _REPRESENTATIVE[kind])
        order = np.asarray(argsort(cost))
        perm[pat] = order
        eq[pat, :-1] = cost[order[:-1]] == cost[order[1:]]
        if pattern_of(5.0 * k + _REPRESENTATIVE[kind]) != pat or not table_fits(perm[pat], eq[pat], cost):
            raise RuntimeError(f'tie table: pattern {pat} does not describe its own representative')
        relabelled = np.unique(cost, return_inverse=True)[1].astype(np.float64)      # the same weak order, other keys
        for other in [relabelled] + [heading_costs(5.0 * k + o) for o in _OTHERS[kind]]:
            if not np.array_equal(np.asarray(argsort(other)), order):
                raise RuntimeError(f"tie table: numpy's argsort is not consistent within pattern {pat} (bin {k}, kind {kind})")
    return perm, eq


def primitive_tables(v_max, dt):
    """th_tab [72, 8] and tt_tab [72, S, 5] of include/d2d_jerk.h, and S, for drone_max_speed `v_max` and step `dt`
    (traj_planner.py:415-440: the parts of generate_primitive that depend on neither the drone nor the goal)"""
    rows, samples = [], []
    for theta in THETAS:
        heading = math.radians(float(theta))
        delt_x = END_DISTANCE * np.cos(heading)
        delt_y = END_DISTANCE * np.sin(heading)
        T = 1.2 * np.linalg.norm(np.array([delt_x, delt_y])) / np.linalg.norm(v_max)
        if not T >= 0.5:
            T = 0.5
        times = int(np.floor(T / dt))
        t = np.arange(dt, times * dt + dt, dt)
        if times < 1 or len(t) < times:
            raise ValueError(f'Jerk_Primitive: heading {theta}: {times} samples, {len(t)} sample times (dt = {dt}): the reference '
                             'indexes past its arrays with these parameters')
        rows.append([delt_x, delt_y, T, T ** 2, T ** 3, T ** 4, T ** 5, float(times)])
        samples.append([[tt, tt ** 2, tt ** 3, tt ** 4, tt ** 5] for tt in t[:times]])
    S = max(len(s) for s in samples)
    if S > A.JERK_MAX_S:
        raise ValueError(f'Jerk_Primitive: {S} samples a primitive (drone_max_speed = {v_max}, dt = {dt}); the device takes at most '
                         f'{A.JERK_MAX_S}')
    tt_tab = np.zeros((len(THETAS), S, A.JERK_TT_F), dtype=np.float64)
    for i, s in enumerate(samples):
        tt_tab[i, :len(s)] = s
    return np.array(rows, dtype=np.float64), tt_tab, S


class JerkState:
    """Tables, per-env state and outputs of one batch, and the ctypes d2d_jerk_call over them and over a BatchState."""

    def __init__(self, params, cfg, device, tracker_radius, tie=None):
        import torch
        self.cfg, self.device = cfg, torch.device(device)
        B, N = cfg.B, cfg.N
        if N > A.JERK_MAX_N:
            raise ValueError(f'Jerk_Primitive on the device: {N} agents per env, at most {A.JERK_MAX_N}')
        self.th_np, self.tt_np, self.S = primitive_tables(params.drone_max_speed, params.dt)
        self.tie_np = tie_table() if tie is None else (np.ascontiguousarray(tie[0], dtype=np.uint8), np.ascontiguousarray(tie[1], dtype=np.uint8))
        if self.tie_np[0].shape != (A.JERK_PATTERNS, A.JERK_NTHETA) or self.tie_np[1].shape != self.tie_np[0].shape:
            raise ValueError(f'tie table: two uint8 arrays [{A.JERK_PATTERNS}, {A.JERK_NTHETA}]')
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)   # noqa: E731
        self.tables = dict(th_tab=up(self.th_np), tt_tab=up(self.tt_np), tie_perm=up(self.tie_np[0]), tie_eq=up(self.tie_np[1]))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)      # noqa: E731
        self.trk_radius0 = z((B, max(N, 1)), torch.float64)
        if N and B:
            self.trk_radius0[:, :N] = torch.as_tensor(np.asarray(tracker_radius, dtype=np.float64)).reshape(B, -1).to(self.device)
        self.t = dict(trk_radius=self.trk_radius0.clone(), trk_prev=z((B, max(N, 1)), torch.uint8),
                      choice=z((B,), torch.int32), stat=z((B,), torch.int32))
        self.scalars = dict(B=B, N=N, S=self.S, W=cfg.W, H=cfg.H, grid_tile=cfg.grid_tile, scale=cfg.scale, W_px=cfg.W_px, H_px=cfg.H_px,
                            drone_radius=float(params.drone_radius), agent_radius=float(params.agent_radius),
                            var_cam=float(params.var_cam), half_v_max=float(0.5 * params.drone_max_speed))

    def call(self, state):
        """the d2d_jerk_call that plans for the envs of BatchState `state`"""
        c = A.JerkCall()
        for k, v in self.scalars.items():
            setattr(c, k, v)
        for k in ('drone', 'target', 'active', 'kf', 'dmap', 'plan_ok', 'wp_valid', 'wp'):
            setattr(c, k, state.t[k].data_ptr() if state.t[k].numel() else None)
        for k, v in dict(self.tables, **self.t).items():
            setattr(c, k, v.data_ptr() if v.numel() else None)
        if self.cfg.N == 0:
            c.active = c.kf = c.trk_radius = c.trk_prev = None
        return c

    def unknown_patterns(self):
        """envs whose latest decision met a tie pattern outside the table (stat bit 1): the known deviation of DESIGN.md section 4"""
        return int((self.t['stat'] & A.JERK_STAT_UNKNOWN).ne(0).sum())
