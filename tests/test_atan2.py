"""csrc/d2d_atan2.h (the atan2 of the LookAhead / LookGoal kernels) compiled for the host, against Python's math.atan2 (CPython's
special cases over libm's atan2) bit for bit.  test_gpu_heading_gaze.py checks the device build.  Expected values come from
libm through a C helper and from math.atan2, never from np.arctan2 (numpy may dispatch its own vectorised atan2)."""
import ctypes as C
import math

import numpy as np
import pytest

import host_build



@pytest.fixture(scope='module')
def atan2_host(tmp_path_factory):
    """(restatement, libm) as numpy functions of (y, x)"""
    lib = host_build.shared('atan2_host.c', tmp_path_factory.mktemp('atan2'), 'libatan2host.so')

    def wrap(f):
        f.argtypes = [C.c_void_p] * 3 + [C.c_int64]

        def call(y, x):
            y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
            out = np.empty_like(y)
            f(y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size)
            return out
        return call
    return wrap(lib.d2d_atan2_host_array), wrap(lib.d2d_atan2_libm_array)


def atan2_pairs(seed=7):
    """1.3e7 (y, x) pairs over every branch of the restatement and the policies' own input shapes"""
    rng = np.random.RandomState(seed)
    ys, xs = [], []

    def add(y, x):
        y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
        ys.append(y.ravel())
        xs.append(x.ravel())

    n = 1_000_000
    sy, sx = rng.choice([-1.0, 1.0], 2 * n), rng.choice([-1.0, 1.0], 2 * n)
    add(sy * 10.0 ** rng.uniform(-30, 30, 2 * n), sx * 10.0 ** rng.uniform(-30, 30, 2 * n))     # many decades
    add(sy[:n] * 10.0 ** rng.uniform(-320, 308, n), sx[:n] * 10.0 ** rng.uniform(-320, 308, n))
    # |y / x| near 1, 2^+-56..60 (the exponent-difference cut-offs), 1/16 and 16 (polynomial / table), tiny
    for r in (1.0, 2.0 ** 60, 2.0 ** -60, 2.0 ** 56, 2.0 ** -56, 2.0 ** 57, 2.0 ** -57, 1 / 16, 16.0, 1e-300, 1e-5):
        x = sx[:n // 4] * rng.uniform(0.5, 2.0, n // 4) * 10.0 ** rng.uniform(-5, 5, n // 4)
        add(sy[:n // 4] * np.abs(x) * r * rng.uniform(0.999, 1.001, n // 4), x)
    # the policies' inputs: velocities in [-60, 60] (some rounded), integer pixel differences in +-1000
    add(rng.uniform(-60, 60, 2 * n), rng.uniform(-60, 60, 2 * n))
    add(np.round(rng.uniform(-60, 60, n), 1), np.round(rng.uniform(-60, 60, n), 1))
    add(np.round(rng.uniform(-60, 60, n)), np.round(rng.uniform(-60, 60, n)))
    add(rng.randint(-1000, 1001, 2 * n).astype(np.float64), rng.randint(-1000, 1001, 2 * n).astype(np.float64))
    add(rng.randint(-1000, 1001, n) + rng.uniform(-1, 1, n), rng.randint(-1000, 1001, n) + rng.uniform(-1, 1, n))
    # +-2000 ulp around both diagonals and both axes, at several magnitudes
    for m in (1.0, 37.5, 1e-3, 1e6):
        w = (np.float64(m).view(np.int64) + np.arange(-2000, 2001)).view(np.float64)          # consecutive doubles around m
        z = np.arange(-2000, 2001) * 5e-324 * m                                                  # ... and around 0
        for s in (-1.0, 1.0):
            add(s * w, m), add(s * w, -m), add(m, s * w), add(-m, s * w)
        add(z, m), add(z, -m), add(m, z), add(-m, z)
    sp = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e308, -1e308, np.inf, -np.inf, np.nan, 0.3, -2.5])
    add(*np.meshgrid(sp, sp))                                                                   # every special combination
    return np.concatenate(ys), np.concatenate(xs)


def same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


@host_build.needs_fma('libm dispatches a non-FMA atan2 variant on this CPU')
def test_atan2_restatement_is_bit_identical_to_libm(atan2_host):
    mine, libm = atan2_host
    y, x = atan2_pairs()
    assert y.size >= 10_000_000
    got = mine(y, x)
    bad = np.flatnonzero(~same_bits(got, libm(y, x)))
    assert bad.size == 0, [(y[i].hex(), x[i].hex(), got[i].hex()) for i in bad[:8]]
    # the helper's expected values are Python's math.atan2: on a sample and on every special case
    idx = np.r_[np.random.RandomState(3).randint(0, y.size, 200_000), np.arange(y.size - 169, y.size)]
    assert same_bits(got[idx], np.array([math.atan2(float(a), float(b)) for a, b in zip(y[idx], x[idx])])).all()


def test_atan2_constants_follow_python():
    assert math.copysign(1.0, math.atan2(-0.0, 0.0)) == -1.0 and math.atan2(-0.0, -0.0) == -math.pi   # LookGoal's atan2(-0., 0.)
    assert (0.75 * math.pi).hex() == '0x1.2d97c7f3321d2p+1' and math.atan2(math.inf, -math.inf) == 0.75 * math.pi
    assert (180.0 / math.pi).hex() == '0x1.ca5dc1a63c1f8p+5' and math.degrees(1.0) == 1.0 * (180.0 / math.pi)
