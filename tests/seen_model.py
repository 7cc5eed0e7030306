"""The time-since-observed map of include/d2d_seen.h restated in numpy: the view test as one whole-array expression over the W x H
grid (the operations and their order are yaw_planner.Oxford.get_view_map's, and numpy's own SIMD arccos decides the cone's edge -- the
thing the device's decision window has to match, so it is never evaluated cell by cell here), the integer bookkeeping of
d2d_seen_update and the crop of envs/training_v3.py:206-209.  Shared by tests/seen_backend.py (the CPU stand-in of the launch),
tests/test_seen_obs_cpu.py and tests/test_gpu_seen_obs.py.  Test infrastructure: the product package never imports this."""
import math

import numpy as np


def view_map(x0, y0, yaw, W, H, scale, depth, view_range):
    """[W, H] bool: the cells whose origin a drone at (x0, y0) with `yaw` degrees sees"""
    scale = int(scale) if float(scale) == int(scale) else float(scale)
    x = np.arange(int(W)).reshape(-1, 1) * scale
    y = np.arange(int(H)).reshape(1, -1) * scale
    r = math.radians(yaw)
    c, s = math.cos(r), -math.sin(r)
    half = math.radians(view_range / 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        d2 = (x0 - x) ** 2 + (y0 - y) ** 2
        q = ((x - x0) * c + (y - y0) * s) / np.sqrt(d2)
        return np.logical_or(d2 <= 0, np.logical_and(np.arccos(q) <= half, d2 <= depth ** 2))


def age_map(seen, call, tab):
    """[W, H] float64: the value of every cell after call `call` -- tab[0][call - seen] where it was seen, tab[1][call] where not"""
    seen = np.asarray(seen).astype(np.int64)
    return np.where(seen > 0, tab[0][call - np.clip(seen, 0, call)], tab[1][call])      # (a record that is no call of the past: as the launch reads it)


def crop(age, x0, y0, L, scale):
    """[L, L] float32: the map zero-padded by (L - 1) / 2 on every side and cut at the drone's cell"""
    edge = (int(L) - 1) // 2
    ix, iy = int(float(x0) // float(scale)), int(float(y0) // float(scale))
    pad = np.pad(np.asarray(age), ((edge, edge), (edge, edge)), 'constant', constant_values=0)
    return pad[ix: ix + L, iy: iy + L].astype(np.float32)


def update(seen, last_call, steps, pose, cfg, view_range, tab):
    """d2d_seen_update for one env: `seen` [W, H] int32 is marked in place.  Returns None where the skip rule holds, else
    (call, refreshed, crop [L, L] float32); the caller stores call as the env's last_call"""
    call = int(steps) + 1
    if call < 1 or call <= int(last_call) or call >= tab.shape[1]:
        return None
    x0, y0, yaw = (float(v) for v in pose[:3])
    view = view_map(x0, y0, yaw, cfg.W, cfg.H, cfg.scale, float(cfg.depth), view_range)
    prev = seen[view]
    refreshed = int(((prev == 0) | (prev < call - 1)).sum())
    seen[view] = call
    return call, refreshed, crop(age_map(seen, call, tab), x0, y0, cfg.L, cfg.scale)
