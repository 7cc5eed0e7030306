"""The swept-trajectory map of include/d2d_swept.h restated in numpy, statement for statement of its semantics: what
Primitive.replan_check returns (traj_planner.py:220-233) from the plugin state as the plan stage of a step finds it, and the crop of
envs/training_v3.py:206-209.  Shared by tests/swept_backend.py (the CPU stand-in of the two launches), tests/test_swept_obs_cpu.py and
tests/test_gpu_swept_obs.py.  Test infrastructure: the product package never imports this."""
from fractions import Fraction

import numpy as np

from drone2d_amd.device_plugins import sq_threshold


def fma_le(dy, dx, lim):
    """fma(dy, dy, dx * dx) <= lim, the fused multiply-add rounded once: decided in plain arithmetic where that cannot differ, exactly
    (rationals, one rounding) where the sum comes within 1e-12 of the limit"""
    p = dx * dx
    approx = dy * dy + p
    if abs(approx - lim) > 1e-12 * max(abs(lim), 1.0):
        return approx <= lim
    return float(Fraction(dy) * Fraction(dy) + Fraction(p)) <= lim


def limits(active, trk_radius, trk_lim, drone_radius):
    """(indices of the active trackers, their squared thresholds): trk_lim where it is cached (> 0), else the threshold of
    drone_radius + trk_radius"""
    ks = [int(k) for k in np.nonzero(np.asarray(active))[0]]
    return ks, [float(trk_lim[k]) if trk_lim[k] > 0 else sq_threshold(float(drone_radius) + float(trk_radius[k])) for k in ks]


def mark(traj, head, stored, kf, active, trk_radius, trk_lim, cfg):
    """(map [W, H] uint8, m).  traj [cap, 4] (x, y, vx, vy), kf [N, >= 4] (the trackers' means first), active / trk_radius / trk_lim
    [N]; cfg: W, H, scale, dt, drone_radius.  Array arithmetic, one rounding per operation as the scalar statements have it; numpy
    fuses nothing"""
    W, H, scale, dt = int(cfg.W), int(cfg.H), float(cfg.scale), float(cfg.dt)
    out = np.zeros((W, H), dtype=np.uint8)
    head = int(head)
    n = max(int(stored) - head, 0)
    if n == 0:
        return out, 0
    ks, lims = limits(active, trk_radius, trk_lim, cfg.drone_radius)
    w = np.asarray(traj, dtype=np.float64)[head:head + n]
    x, y = w[:, 0], w[:, 1]
    ti = np.arange(n, dtype=np.float64) * dt                      # i * dt
    m = n
    if ks:
        mu, lim = np.asarray(kf, dtype=np.float64)[ks], np.asarray(lims, dtype=np.float64)[None, :]
        ex, ey = mu[None, :, 0] + ti[:, None] * mu[None, :, 2], mu[None, :, 1] + ti[:, None] * mu[None, :, 3]   # estimate_pos(i * dt)
        dx, dy = ex - x[:, None], ey - y[:, None]
        approx = dy * dy + dx * dx
        hit = approx <= lim
        for i, q in zip(*np.nonzero(np.abs(approx - lim) <= 1e-12 * np.maximum(np.abs(lim), 1.0))):
            hit[i, q] = fma_le(float(dy[i, q]), float(dx[i, q]), float(lim[0, q]))
        rows = np.nonzero(hit.any(axis=1))[0]
        if len(rows):
            m = int(rows[0]) + 1                                  # the hit waypoint's cell was written before the test
    ci, cj = np.floor_divide(x[:m], scale).astype(np.int64), np.floor_divide(y[:m], scale).astype(np.int64)
    val = (ti[:m].astype(np.int64) & 0xff).astype(np.uint8)      # trunc(i * dt) as uint8
    inside = (ci >= 0) & (ci < W) & (cj >= 0) & (cj < H)
    for a, b, v in zip(ci[inside], cj[inside], val[inside]):      # in order: the last write to a cell stands
        out[a, b] = v
    return out, m


def crop(full, drone_xy, cfg):
    """[L, L]: the map zero-padded by 2 * (depth // scale) = (L - 1) / 2 on every side, cut at the drone's cell"""
    L, scale = int(cfg.L), float(cfg.scale)
    edge = (L - 1) // 2
    ix, iy = int(float(drone_xy[0]) // scale), int(float(drone_xy[1]) // scale)
    pad = np.pad(np.asarray(full), ((edge, edge), (edge, edge)), 'constant', constant_values=0)
    return pad[ix: ix + L, iy: iy + L].astype(np.uint8)


def mark_env(env, e, plugins=None):
    """mark() on env e of a VecDrone2DEnv (or on a snapshot dict of its plugin tensors given as `plugins`)"""
    t = plugins if plugins is not None else {k: v[e].cpu().numpy() for k, v in env.plugins.t.items()
                                             if k in ('traj', 'traj_hdr', 'trk_radius', 'trk_lim')}
    if plugins is None:
        t['kf'], t['active'] = env.state.kf[e].cpu().numpy(), env.state.active[e].cpu().numpy()
    N = env.cfg.N
    head, stored = (int(v) for v in t['traj_hdr'])
    return mark(t['traj'], head, stored, t['kf'].reshape(-1, t['kf'].shape[-1])[:N], t['active'][:N], t['trk_radius'][:N],
                t['trk_lim'][:N], env.cfg)
