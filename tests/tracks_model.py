"""The tracker-forecast map of include/d2d_tracks.h restated in numpy: the definition over the whole W x H grid, then the pad and the
cut of envs/training_v3.py:206-209 -- no bounding boxes, no window arithmetic, so it shares nothing with the code under test but the
definition.  Array arithmetic, one rounding per operation as the scalar statements have it (numpy fuses nothing); the one fused
multiply-add of the distance test is decided exactly where it could matter (swept_model.fma_le).  Shared by tests/tracks_backend.py
(the CPU stand-in of the launch), tests/test_tracks_obs_cpu.py and tests/test_gpu_tracks_obs.py.  Test infrastructure: the product
package never imports this."""
import numpy as np

from drone2d_amd.device_plugins import sq_threshold
from swept_model import fma_le


def forecast_map(mu, active, radius, W, H, scale, dt, drone_radius, margin, samples):
    """F [W, H] int32: 1 + the first sample k at which an active tracker's estimate_pos(k * dt) is within its threshold of the
    cell's centre, 0 = none.  mu [N, >= 4], active [N], radius [N]"""
    W, H, scale, dt = int(W), int(H), float(scale), float(dt)
    F = np.zeros((W, H), dtype=np.int32)
    px = (scale * (np.arange(W, dtype=np.float64) + 0.5))[:, None]          # get_real_pos, utils.py:543
    py = (scale * (np.arange(H, dtype=np.float64) + 0.5))[None, :]
    mu = np.asarray(mu, dtype=np.float64)
    for q in np.nonzero(np.asarray(active))[0]:
        thr = float(drone_radius) + float(radius[q]) + float(margin)
        lim = sq_threshold(thr)
        if not lim >= 0.0:
            continue
        for k in range(int(samples) - 1, -1, -1):                           # descending: the smaller k is written last
            t = k * dt
            ex, ey = mu[q, 0] + t * mu[q, 2], mu[q, 1] + t * mu[q, 3]       # estimate_pos, utils.py:220-223
            with np.errstate(all='ignore'):
                dx, dy = px - ex, py - ey
                approx = dy * dy + dx * dx
                hit = approx <= lim
                close = np.abs(approx - lim) <= 1e-12 * max(abs(lim), 1.0)
            for i, j in zip(*np.nonzero(close)):
                hit[i, j] = fma_le(float(dy[0, j]), float(dx[i, 0]), lim)
            F[hit & ((F == 0) | (F > k + 1))] = k + 1
    return F


def crop(F, x0, y0, L, scale):
    """[L, L] uint8: the map zero-padded by (L - 1) / 2 on every side and cut at the drone's cell"""
    edge = (int(L) - 1) // 2
    ix, iy = int(float(x0) // float(scale)), int(float(y0) // float(scale))
    pad = np.pad(np.asarray(F), ((edge, edge), (edge, edge)), 'constant', constant_values=0)
    return pad[ix: ix + L, iy: iy + L].astype(np.uint8)


def window(pose, mu, active, radius, cfg, margin, samples):
    """the L x L window of an env's forecast map; cfg: W, H, L, scale, dt, drone_radius"""
    F = forecast_map(mu, active, radius, cfg.W, cfg.H, cfg.scale, cfg.dt, cfg.drone_radius, margin, samples)
    return crop(F, pose[0], pose[1], cfg.L, cfg.scale)


def update(win, cells, last_step, steps, pose, mu, active, radius, cfg, margin, samples, force=0):
    """d2d_tracks_update for one env.  Returns None where the skip rule holds, else (window [L, L] uint8, cells, last_step)"""
    if not force and int(steps) == int(last_step):
        return None
    w = window(pose, mu, active, radius, cfg, margin, samples)
    return w, int((w != 0).sum()), int(steps)
