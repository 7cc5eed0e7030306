"""NumPy model of the renderer, written from the text of include/d2d_render.h and from nothing else: the display list of a slot's
state, and the pixels of a display list over a cell layer.  float64 throughout; numpy fuses no multiply-add, so every operator is
one IEEE operation as the header demands.  Test infrastructure: the product package never imports this."""
import math

import numpy as np

DISC, LINE, ARC, POLY = 1, 2, 3, 4
GEOM = 20
GREY = {1: 100, 2: 200, 3: 200}       # OCCUPIED; UNOCCUPIED and DYNAMIC; everything else (UNEXPLORED) is 240


def radians(a):
    return a * (math.pi / 180.0)


def _item(kind, rgb, width, geom, npts=0):
    g = np.zeros(GEOM)
    g[:len(geom)] = geom
    return (kind, tuple(rgb), float(width), int(npts), g)


def disc(rgb, cx, cy, r):
    return _item(DISC, rgb, 0.0, [cx, cy, r])


def line(rgb, ax, ay, bx, by, width=2.0):
    return _item(LINE, rgb, width, [ax, ay, bx, by])


def arc(rgb, x, y, R, yaw, view_range, width=2.0):
    """the view arc of a drone at (x, y) heading `yaw` degrees"""
    start, stop = radians(yaw - view_range / 2), radians(yaw + view_range / 2)
    return _item(ARC, rgb, width, [x - R, y - R, 2 * R, 2 * R, start, stop, math.cos(start), math.sin(start), math.cos(stop), math.sin(stop),
                                   view_range])


def poly(rgb, points):
    pts = [float(v) for p in points for v in p]
    return _item(POLY, rgb, 0.0, pts, len(pts) // 2)


def pack(items):
    """a list of items as the arrays of a display list"""
    n = len(items)
    return dict(kind=np.array([i[0] for i in items], dtype=np.int32).reshape(n), rgb=np.array([i[1] for i in items], dtype=np.uint8).reshape(n, 3),
                width=np.array([i[2] for i in items], dtype=np.float64).reshape(n), npts=np.array([i[3] for i in items], dtype=np.uint8).reshape(n),
                geom=np.array([i[4] for i in items], dtype=np.float64).reshape(n, GEOM), count=n)


def make_list(drone, agents, active, vel, target, pillars, traj, R, view_range, drone_radius, steps=1, n_seeded=0):
    """the display list of one slot.  drone: x, y, yaw; agents [6, N] (x, y, preferred vx, vy, radius, .); vel [2, N] or None;
    pillars [P, 3]; traj [n, 2] or None"""
    x, y, yaw = (float(v) for v in drone[:3])
    g = (100, 100, 100)
    start, stop = radians(yaw - view_range / 2), radians(yaw + view_range / 2)
    out = [arc(g, x, y, R, yaw, view_range)]
    for a in (stop, start):
        out.append(line(g, x, y, x + R * math.cos(a), y - R * math.sin(a)))
    dx, dy = 5 * math.cos(radians(yaw + 45)), -5 * math.sin(radians(yaw + 45))
    out += [line(g, x - dx, y - dy, x + dx, y + dy), line(g, x - dy, y + dx, x + dy, y - dx)]
    for cx, cy in ((x - dx, y - dy), (x + dx, y + dy), (x - dy, y + dx), (x + dy, y - dx)):
        out.append(disc(g, float(int(cx)), float(int(cy)), 3.5))
    for p in np.asarray(pillars).reshape(-1, 3):
        out.append(disc((130, 130, 130), float(p[0]), float(p[1]), float(p[2])))
    if traj is not None and len(traj) > 1:
        t = np.asarray(traj, dtype=np.float64).reshape(-1, 2)
        for a, b in zip(t[:-1], t[1:]):
            out.append(line((0, 0, 0), a[0], a[1], b[0], b[1]))
    N = agents.shape[1]
    for k in range(N):
        px, py = agents[0, k], agents[1, k]
        if vel is not None:
            vx, vy = vel[0, k], vel[1, k]
        elif steps == 0 and k < n_seeded:
            vx, vy = 0.0, 0.0
        else:
            vx, vy = agents[2, k], agents[3, k]
        cx, cy = np.rint(px), np.rint(py)
        out.append(disc((130, 176, 210) if active[k] else (200, 36, 35), cx, cy, np.rint(agents[4, k])))
        out.append(line((53, 53, 53), cx, cy, np.rint(px + vx), np.rint(py + vy)))
    pts = []
    for i in range(10):
        r = drone_radius if i % 2 == 0 else drone_radius * 0.5
        pts.append((target[0] + r * math.sin(math.pi / 5 * i), target[1] - r * math.cos(math.pi / 5 * i)))
    out.append(poly((0, 0, 150), pts))
    return pack(out)


# ---------------------------------------------------------------------------------------------------------------- pixels
def cell_layer(cells, W_px, H_px, scale, d=1):
    """[Hf, Wf, 3] uint8: pixel (x, y) = (u d, v d) takes the colour of cell (x // scale, y // scale) of cells [W, H] (grid codes);
    a pixel beyond the last cell is UNEXPLORED"""
    xs, ys = np.arange(0, W_px, d), np.arange(0, H_px, d)
    i, j = xs // scale, ys // scale
    W, H = cells.shape
    code = np.zeros((len(ys), len(xs)), dtype=np.uint8)
    ok_i, ok_j = i < W, j < H
    code[np.ix_(ok_j, ok_i)] = cells[np.ix_(i[ok_i], j[ok_j])].T
    grey = np.full(code.shape, 240, dtype=np.uint8)
    for c, v in GREY.items():
        grey[code == c] = v
    return np.repeat(grey[:, :, None], 3, axis=2)


def covers(kind, width, npts, g, X, Y):
    """the mask of the sample points (X, Y) the item covers"""
    with np.errstate(invalid='ignore', over='ignore'):
        if kind == DISC:
            dx, dy = X - g[0], Y - g[1]
            return dx * dx + dy * dy <= g[2] * g[2]
        if kind == LINE:
            h = width * 0.5
            h2 = h * h
            apx, apy, abx, aby = X - g[0], Y - g[1], g[2] - g[0], g[3] - g[1]
            t, l2 = apx * abx + apy * aby, abx * abx + aby * aby
            at_a = (apx * apx + apy * apy) <= h2
            bx, by = X - g[2], Y - g[3]
            at_b = (bx * bx + by * by) <= h2
            c = abx * apy - aby * apx
            mid = c * c <= h2 * l2
            if l2 == 0.0:
                return at_a
            return np.where(t <= 0.0, at_a, np.where(t >= l2, at_b, mid))
        if kind == ARC:
            R = g[2] * 0.5
            cx, cy = g[0] + R, g[1] + g[3] * 0.5
            dx, ey = X - cx, -(Y - cy)
            q = dx * dx + ey * ey
            ri = max(R - width, 0.0)
            ring = (ri * ri <= q) & (q <= R * R)
            if g[10] >= 360.0:
                return ring
            a, b = g[6] * ey - g[7] * dx >= 0.0, g[8] * ey - g[9] * dx <= 0.0
            return ring & ((a & b) if g[10] <= 180.0 else (a | b))
        if kind == POLY:
            inside = np.zeros(X.shape, dtype=bool)
            if not 3 <= npts <= 10:
                return inside
            for i in range(npts):
                j = (i - 1) % npts
                xi, yi, xj, yj = g[2 * i], g[2 * i + 1], g[2 * j], g[2 * j + 1]
                dy = yj - yi
                lhs, rhs = (X - xi) * dy, (xj - xi) * (Y - yi)
                counts = ((yi > Y) != (yj > Y)) & ((lhs < rhs) if dy > 0.0 else (lhs > rhs))
                inside ^= counts
            return inside
    return np.zeros(X.shape, dtype=bool)


def raster(lst, cells, W_px, H_px, scale, d=1):
    """[Hf, Wf, 3] uint8: the cell layer under the list's first `count` items in order, the last one that covers a pixel winning"""
    frame = cell_layer(cells, W_px, H_px, scale, d)
    xs, ys = np.arange(0, W_px, d, dtype=np.float64), np.arange(0, H_px, d, dtype=np.float64)
    X, Y = np.meshgrid(xs, ys)
    for k in range(int(lst['count'])):
        m = covers(int(lst['kind'][k]), float(lst['width'][k]), int(lst['npts'][k]), lst['geom'][k], X, Y)
        frame[m] = lst['rgb'][k]
    return frame
