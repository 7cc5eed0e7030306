"""Shared arguments of the asin tests (test_asin.py on the host build, test_gpu_asin.py on the device): every branch of
csrc/metrics/d2d_asin.h, its cuts, the velocity-obstacle metric's own argument shape and the special values."""
import math

import numpy as np

# |x| at which d2d_asin changes its branch: 2^-26, 1/8, 1/4, 1/2, 3/4, 59/64, 61/64, 31/32, 1
CUTS = (2.0 ** -26, 0.125, 0.25, 0.5, 0.75, 0.921875, 0.953125, 0.96875, 1.0)
ULP1 = 2.0 ** -52
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 1.0 + ULP1, -1.0 - ULP1, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308,
                     -2.2250738585072014e-308, 1e-310, -1e-310, 2.0, -2.0, 1e300, -1e300])


def neighbours(v, n=2000):
    """the 2 n + 1 consecutive doubles around v > 0"""
    return (np.float64(v).view(np.int64) + np.arange(-n, n + 1)).view(np.float64)


def cut_neighbourhoods(n=2000):
    w = np.concatenate([neighbours(c, n) for c in CUTS])
    return np.concatenate([w, -w])


def per_branch(rng, n):
    """n uniform arguments in each of the eight branch ranges between the CUTS, in each sign"""
    out = []
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        u = rng.uniform(lo, hi, n)
        out += [u, -rng.uniform(lo, hi, n)]
    return np.concatenate(out)


def vo_shaped(rng, n):
    """(5 + r) / sqrt(fma(dy, dy, dx * dx)) as d2d_vo_geometry forms it, for integer pixel offsets (the sum of squares is exact,
    fused or not) and fractional ones (numpy's unfused sum: a last-bit neighbour of the fused one); only the quotients a cone is
    built from (<= 1)"""
    out = []
    for frac in (False, True):
        dx, dy = rng.randint(-480, 481, n).astype(np.float64), rng.randint(-480, 481, n).astype(np.float64)
        if frac:
            dx, dy = dx + rng.uniform(-1, 1, n), dy + rng.uniform(-1, 1, n)
        r = rng.uniform(5, 15, n) if frac else rng.choice([5.0, 10.0, 15.0, 7.0], n)
        dist = np.sqrt(dy * dy + dx * dx)
        q = (5.0 + r)[dist > 0] / dist[dist > 0]
        out.append(q[q <= 1.0])
    return np.concatenate(out)


def math_asin(x):
    """math.asin over a flat array, NaN written by hand where it raises (|x| > 1) and for NaN"""
    return np.array([float('nan') if (v != v or v > 1.0 or v < -1.0) else math.asin(v) for v in x.tolist()], dtype=np.float64)


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))
