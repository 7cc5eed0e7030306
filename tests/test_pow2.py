"""csrc/d2d_pow2.h (the pow(x, 2.0) of the Owl gaze stage) compiled for the host, against libm's pow bit for bit; with -m gpu the
device build (d2d_pow2_array) against the host build on the same arguments.  Expected values come from libm through a C helper,
never from numpy's `**` on arrays (numpy squares arrays with a multiplication)."""
import ctypes as C
import platform

import numpy as np
import pytest

from test_atan2 import same_bits
import host_build

needs_glibc_235 = pytest.mark.skipif(platform.libc_ver()[0] != 'glibc' or platform.libc_ver()[1] != '2.35',
                                     reason=f'd2d_pow2.h restates the pow of glibc 2.35; this host has {platform.libc_ver()}')
needs_fma = host_build.needs_fma('libm dispatches a non-FMA pow variant on this CPU')


@pytest.fixture(scope='module')
def pow2_host(tmp_path_factory):
    """(restatement, libm) as numpy functions of x"""
    lib = host_build.shared('pow2_host.c', tmp_path_factory.mktemp('pow2'), 'libpow2host.so')

    def wrap(f):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]

        def call(x):
            x = np.ascontiguousarray(x, np.float64)
            out = np.empty_like(x)
            f(x.ctypes.data, out.ctypes.data, x.size)
            return out
        return call
    return wrap(lib.d2d_pow2_host_array), wrap(lib.d2d_pow2_libm_array)


def pow2_args(seed=23):
    """1.2e7 arguments: the Owl stage's range (a speed / 10), every binade from the subnormals to overflow, the thresholds of the
    restatement's branches, and the special values"""
    rng = np.random.RandomState(seed)
    parts = [rng.uniform(0.0, 8.0, 6_000_000),                                   # norm(velocity / 10), speeds up to 80 px / s
             2.0 ** rng.uniform(-1075, 1024, 5_000_000),                        # log-uniform: subnormal x up to x^2 = inf
             2.0 ** rng.uniform(-540, -360, 500_000),                            # x^2 subnormal or about to be (exp's special case)
             2.0 ** rng.uniform(360, 513, 500_000)]                              # x^2 near the overflow threshold
    for m in (1.0, 0.5, 2.0, float.fromhex('0x1.69555p-1'), float.fromhex('0x1.69555p0'), 2.0 ** -511, 2.0 ** -537, 2.0 ** 512, 2.0 ** -1022, 2.0 ** 256):
        parts.append((np.float64(m).view(np.int64) + np.arange(-2000, 2001)).view(np.float64))    # consecutive doubles around m
    parts.append(np.arange(0, 4001) * 5e-324)                                    # the smallest subnormals
    parts.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, -2.5, 1.7976931348623157e308, 5e-324]))
    return np.concatenate(parts)


@needs_glibc_235
@needs_fma
def test_pow2_restatement_is_bit_identical_to_libm(pow2_host):
    mine, libm = pow2_host
    x = pow2_args()
    assert x.size >= 10_000_000
    want = libm(x)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        not_square = int(np.count_nonzero(~same_bits(want, x * x)))
    assert not_square >= 1000, not_square              # the arguments on which an `x * x` shortcut fails
    got = mine(x)
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]
    # the helper's expected values are what numpy's scalar power gives (the reference's `np.float64 ** 2`)
    idx = np.r_[np.random.RandomState(3).randint(0, 6_000_000, 100_000), np.arange(x.size - 10, x.size)]
    with np.errstate(all='ignore'):
        assert same_bits(want[idx], np.array([float(np.float64(v) ** 2) for v in x[idx]])).all()


@pytest.mark.gpu
@needs_glibc_235
@needs_fma
def test_device_pow2_is_bit_identical_to_the_host_build(hip, pow2_host):
    import torch
    x = pow2_args()
    want = pow2_host[0](x)
    xd = torch.from_numpy(x).to(hip.device)
    out = torch.empty_like(xd)
    hip.pow2_array(xd, out)
    got = out.cpu().numpy()
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]
