"""The per-ray scan of include/d2d_scan.h restated in plain Python floats from its definition: Raycast.castRay's loop (math.tan, the
iterated sums, `//` for the cell, the agent test in front of the wall test at every sample) with the record of include/d2d_scan.h
as its result.  Shared by tests/scan_backend.py (the CPU stand-in of the launch), tests/test_scan_obs_cpu.py and
tests/test_gpu_scan_obs.py.  Test infrastructure: the product package never imports this."""
import math

import numpy as np

WALL_OF_KIND = (0, 1, 0, 2)        # the port's 'wall' (include/d2d_scan.h: the one deviation)


def positive_angle(angle):
    angle = math.copysign(abs(angle) % (math.pi * 2), angle)
    if angle < 0:
        angle += math.pi * 2
    return angle


def grid_index(i, j, H, tile):
    """byte of cell (i, j) in one env's grid under d2d_cfg.grid_tile"""
    if tile:
        return (((i >> 4) * ((H + 15) >> 4) + (j >> 4)) << 8) | ((i & 15) << 4) | (j & 15)
    return i * H + j


def cast_ray(x0, y0, yaw, ray_angle, scale, W_px, H_px, depth, occupied, agents):
    """One ray.  `occupied(i, j)`: is the cell OCCUPIED; `agents`: [(px, py, r2)].  Returns (x_hit, y_hit, kind, hit list, range)"""
    step = scale - 1
    ang = positive_angle((math.pi * 2 - yaw * (math.pi / 180)) + ray_angle)
    faced_right = ang < math.radians(90) or ang > math.radians(270)
    faced_up = ang > math.pi
    slope = math.tan(ang)
    if abs(slope) > 1:
        slope = 1 / slope
        ys = -step if faced_up else step
        xs = ys * slope
    else:
        xs = step if faced_right else -step
        ys = xs * slope
    x, y = x0, y0
    hits, kind, last = [0] * len(agents), 0, None
    while 0 < x < W_px and 0 < y < H_px:
        last = (x, y)
        for k, (px, py, r2) in enumerate(agents):
            if (px - x) ** 2 + (py - y) ** 2 <= r2:
                hits[k] = 1
        if any(hits):
            kind = 2
            break
        dist = (x - x0) ** 2 + (y - y0) ** 2
        if occupied(int(x // scale), int(y // scale)):
            kind = 1
            break
        if dist >= depth ** 2:
            kind = 3
            break
        x = x + xs
        y = y + ys
    rng = 0.0 if last is None else math.sqrt((last[0] - x0) ** 2 + (last[1] - y0) ** 2)
    return (last[0], last[1], kind, hits, rng) if kind else (-1.0, -1.0, 0, hits, rng)


def scan(pose, agents, gt, cfg, words, far=False):
    """d2d_scan_update for one env that is due: `pose` (x, y, yaw), `agents` [AF, N] planes, `gt` the env's grid bytes in the cfg's
    layout.  Returns end [R, 2] float64, kind [R] uint8, hit [R, words] uint32, obs [2, R] float32.  `far`: for the large cases an agent
    farther from the drone than its radius + depth + 3 * scale -- no sample comes within a cell of that -- is left out beforehand
    instead of being tested at every sample"""
    R, N = cfg.R, cfg.N
    x0, y0, yaw = (float(v) for v in pose[:3])
    scale = float(cfg.scale)
    flat = np.asarray(gt).reshape(-1)
    ag = [(float(agents[0, k]), float(agents[1, k]), float(agents[5, k])) for k in range(N)]
    if far:
        reach = lambda r2: math.sqrt(max(r2, 0.0)) + float(cfg.depth) + 3 * scale      # noqa: E731
        keep = [not (math.hypot(px - x0, py - y0) > reach(r2)) for px, py, r2 in ag]
        skip = [k for k in range(N) if not keep[k]]
        near = [k for k in range(N) if keep[k]]
        end, kind, hit, obs = _scan([ag[k] for k in near], x0, y0, yaw, scale, flat, cfg, words)
        if skip:                                   # the near agents' bits go back to their own places
            full = np.zeros_like(hit)
            for q, k in enumerate(near):
                full[:, k >> 5] |= ((hit[:, q >> 5] >> np.uint32(q & 31)) & np.uint32(1)) << np.uint32(k & 31)
            hit = full
        return end, kind, hit, obs
    return _scan(ag, x0, y0, yaw, scale, flat, cfg, words)


def _scan(ag, x0, y0, yaw, scale, flat, cfg, words):
    R = cfg.R
    W, H, tile = cfg.W, cfg.H, cfg.grid_tile
    occupied = lambda i, j: flat[grid_index(min(max(i, 0), W - 1), min(max(j, 0), H - 1), H, tile)] == 1      # noqa: E731
    end, kind = np.zeros((R, 2), dtype=np.float64), np.zeros(R, dtype=np.uint8)
    hit, obs = np.zeros((R, words), dtype=np.uint32), np.zeros((2, R), dtype=np.float32)
    for i in range(R):
        x, y, k, hits, rng = cast_ray(x0, y0, yaw, float(cfg.ray_off0) + float(cfg.ray_dth) * i, scale, float(cfg.W_px), float(cfg.H_px),
                                      float(cfg.depth), occupied, ag)
        end[i], kind[i] = (x, y), k
        for a, h in enumerate(hits):
            if h:
                hit[i, a >> 5] |= np.uint32(1 << (a & 31))
        obs[0, i], obs[1, i] = np.float32(rng), np.float32(k)
    return end, kind, hit, obs


def update(last_step, steps, pose, agents, gt, cfg, words):
    """None where the skip rule holds, else scan(...)"""
    if int(steps) < 1 or int(steps) == int(last_step):
        return None
    return scan(pose, agents, gt, cfg, words)
