"""csrc/d2d_tan.h (the tan the HIP kernels use) compiled for the host, against the libm tan that the
reference's math.tan resolves to: bit for bit.  The device build is checked in test_gpu_parity.py."""
import ctypes as C
import math

import numpy as np
import pytest

import host_build


@pytest.fixture(scope='module')
def tan_host(tmp_path_factory):
    lib = host_build.shared('tan_host.c', tmp_path_factory.mktemp('tan'), 'libtanhost.so')
    lib.d2d_tan_host_array.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]

    def f(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        lib.d2d_tan_host_array(x.ctypes.data, out.ctypes.data, x.size)
        return out
    return f


@host_build.needs_fma('libm dispatches a non-FMA tan variant on this CPU')
def test_tan_restatement_is_bit_identical_to_libm(tan_host):
    rng = np.random.RandomState(11)
    xs = [rng.uniform(0, 2 * np.pi, 3_000_000), rng.uniform(-25, 25, 1_500_000), rng.uniform(-0.8, 0.8, 1_000_000),
          rng.uniform(-0.07, 0.07, 500_000), rng.uniform(-2e-8, 2e-8, 100_000), np.array([0.0, -0.0, 25.0, -25.0])]
    for k in range(-8, 9):      # neighbourhoods of every multiple of pi/4: the structured ray angles
        c = k * math.pi / 4
        lo = c
        for _ in range(300):
            lo = np.nextafter(lo, -np.inf)
        v = [lo]
        for _ in range(600):
            v.append(np.nextafter(v[-1], np.inf))
        xs.append(np.array(v))
    x = np.concatenate(xs)
    want = np.array([math.tan(v) for v in x[:200000]])            # Python's math.tan on a slice ...
    got = tan_host(x)
    assert np.array_equal(got[:200000].view(np.int64), want.view(np.int64))
    want_all = np.tan(x[-(17 * 601 + 4):])                        # ... numpy on the structured block (same libm? checked below)
    libm = C.CDLL('libm.so.6')
    libm.tan.restype = C.c_double
    libm.tan.argtypes = [C.c_double]
    idx = rng.randint(0, x.size, 300000)
    ref = np.array([libm.tan(float(v)) for v in x[idx]])
    assert np.array_equal(got[idx].view(np.int64), ref.view(np.int64))
    tail = x[-(17 * 601 + 4):]
    ref_tail = np.array([libm.tan(float(v)) for v in tail])
    assert np.array_equal(got[-tail.size:].view(np.int64), ref_tail.view(np.int64))


def test_reference_ray_angle_pipeline_constants():
    """Constants the kernels hard-code are the doubles Python computes (utils.py:594,614-618,636-637)."""
    assert (math.pi * 2).hex() == '0x1.921fb54442d18p+2'
    assert (math.pi / 180).hex() == '0x1.1df46a2529d39p-6' and math.radians(270) == 270 * (math.pi / 180)
    assert math.radians(270).hex() == '0x1.2d97c7f3321d2p+2' and math.radians(90).hex() == '0x1.921fb54442d18p+0'
    assert math.cos(math.pi / 6).hex() == '0x1.bb67ae8584cabp-1' and math.sin(math.pi / 6).hex() == '0x1.fffffffffffffp-2'
