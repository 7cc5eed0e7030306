"""csrc/d2d_log.h (the log of the measurement noise's Gaussian draw) compiled for the host, against libm's log bit for bit; with
-m gpu the device build (d2d_log_array) against the host build on the same arguments."""
import ctypes as C
import math
import platform

import numpy as np
import pytest

from test_atan2 import same_bits
import host_build

needs_glibc_235 = pytest.mark.skipif(platform.libc_ver()[0] != 'glibc' or platform.libc_ver()[1] != '2.35',
                                     reason=f'd2d_log.h restates the log of glibc 2.35; this host has {platform.libc_ver()}')
needs_fma = host_build.needs_fma('libm dispatches a non-FMA log variant on this CPU')


@pytest.fixture(scope='module')
def log_host(tmp_path_factory):
    """(restatement, libm) as numpy functions of x"""
    lib = host_build.shared('log_host.c', tmp_path_factory.mktemp('log'), 'libloghost.so', extra=['-fno-builtin'])

    def wrap(f):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]

        def call(x):
            x = np.ascontiguousarray(x, np.float64)
            out = np.empty_like(x)
            f(x.ctypes.data, out.ctypes.data, x.size)
            return out
        return call
    return wrap(lib.d2d_log_host_array), wrap(lib.d2d_log_libm_array)


LO, HI = 1.0 - 2.0 ** -4, 1.0 + float.fromhex('0x1.09p-4')      # the near-1 branch is [LO, HI)


def log_args(seed=29):
    """1.25e7 arguments: (0, 1) densely (the range of the polar method's r2), the near-1 branch from both sides and across its
    thresholds, every binade from the subnormals up, consecutive doubles around the branch points, and the special values"""
    rng = np.random.RandomState(seed)
    parts = [rng.random_sample(6_000_000),                                       # r2 = x1^2 + x2^2 < 1
             rng.uniform(LO - 0.01, HI + 0.01, 2_000_000),                       # the near-1 branch and a margin on either side
             1.0 + rng.choice([-1.0, 1.0], 500_000) * 2.0 ** rng.uniform(-53, -4, 500_000),   # towards 1, every magnitude of x - 1
             2.0 ** rng.uniform(-1075, 1024, 4_000_000)]                        # log-uniform: every binade, subnormals included
    for m in (1.0, LO, HI, 0.5, 2.0, float.fromhex('0x1.6p-1'), float.fromhex('0x1.6p0'), 2.0 ** -1022, 2.0 ** -1021,
              1.7976931348623157e308, math.e):
        parts.append((np.float64(m).view(np.int64) + np.arange(-2000, 2001)).view(np.float64))    # consecutive doubles around m
    rows = (np.float64(float.fromhex('0x1.6p-1')).view(np.int64) + (np.arange(128, dtype=np.int64) << 45))
    parts.append((rows[:, None] + np.arange(-3, 4)[None, :]).ravel().view(np.float64))            # both sides of every table row's edge
    parts.append(np.arange(0, 4001) * 5e-324)                                    # the smallest subnormals
    parts.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, -2.5, -5e-324, 1.7976931348623157e308, 5e-324]))
    return np.concatenate(parts)


@needs_glibc_235
@needs_fma
def test_log_restatement_is_bit_identical_to_libm(log_host):
    mine, libm = log_host
    x = log_args()
    assert x.size >= 10_000_000
    near = int(np.count_nonzero((x >= LO) & (x < HI)))
    assert near >= 1_000_000, near                     # the polynomial branch is exercised, not only touched
    want = libm(x)
    got = mine(x)
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]
    # the helper's expected values are what Python's math.log gives (the same libm entry numpy's legacy Gaussian calls)
    idx = np.random.RandomState(3).randint(0, 8_000_000, 100_000)
    assert same_bits(want[idx], np.array([math.log(v) if v > 0 else -np.inf for v in x[idx]])).all()


@pytest.mark.gpu
@needs_glibc_235
@needs_fma
def test_device_log_is_bit_identical_to_the_host_build(hip, log_host):
    import torch
    x = log_args()
    want = log_host[0](x)
    xd = torch.from_numpy(x).to(hip.device)
    out = torch.empty_like(xd)
    hip.log_array(xd, out)
    got = out.cpu().numpy()
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]
