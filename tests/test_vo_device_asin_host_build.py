"""The velocity-obstacle cones with the half angle taken by csrc/metrics/d2d_asin.h (d2d_vo_cones_arg_seq of d2d_vo.h) compiled for
the host with gcc, against the Python model and against d2d_vo_cones_seq fed with metrics.host_asin, bit for bit.  A second,
stand-alone build runs the loop and d2d_asin under AddressSanitizer and UBSan as a program of its own: no index leaves either
table.  test_gpu_vo_device_asin.py checks the device build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vo_cases
from drone2d_amd import metrics
import host_build

CSRC = os.path.join(host_build.CSRC, 'metrics')
needs_fma = host_build.needs_fma('libm dispatches non-FMA asin / sin / cos / atan2 variants on this CPU')


@pytest.fixture(scope='module')
def vo_host(tmp_path_factory):
    lib = host_build.shared('vo_asin_host.c', tmp_path_factory.mktemp('vo_asin'), 'libvoasinhost.so', include=CSRC)
    V, I = C.c_void_p, C.c_int32
    lib.vo_host_geometry.argtypes = [V, V, C.c_double, I, I, I, V, V, V]
    lib.vo_host_cones.argtypes = [V, V, V, I, I, I, V]
    lib.vo_host_cones_arg.argtypes = [V, V, V, I, I, I, V, V]
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_host(lib, agents, pos, rA=5.0):
    """one world, agents [6, N]: half and cone of d2d_vo_cones_arg_seq (poisoned buffers), the cone without half_out, and the
    cone of d2d_vo_cones_seq fed with host_asin"""
    agents, pos = np.ascontiguousarray(agents, np.float64), np.ascontiguousarray(pos, np.float64)
    N, P = agents.shape[1], len(pos)
    arg, tba = np.full((P, N), np.nan), np.full((P, N), np.nan)
    col = np.full(P, 0x7f, np.uint8)
    lib.vo_host_geometry(agents.ctypes.data, pos.ctypes.data, rA, 1, N, P, arg.ctypes.data, tba.ctypes.data, col.ctypes.data)
    half = np.full((P, N), np.nan)
    cone, cone_null, cone_host = (np.full((P, N, 2), np.nan) for _ in range(3))
    lib.vo_host_cones_arg(tba.ctypes.data, arg.ctypes.data, col.ctypes.data, 1, N, P, half.ctypes.data, cone.ctypes.data)
    lib.vo_host_cones_arg(tba.ctypes.data, arg.ctypes.data, col.ctypes.data, 1, N, P, None, cone_null.ctypes.data)
    host_half = metrics.host_asin(arg)
    lib.vo_host_cones(tba.ctypes.data, host_half.ctypes.data, col.ctypes.data, 1, N, P, cone_host.ctypes.data)
    return dict(arg=arg, collided=col, half=half, cone=cone, cone_null=cone_null, host_half=host_half, cone_host=cone_host)


def assert_same(got, want):
    assert np.array_equal(got['collided'], want['collided'])
    assert (bits(got['arg']) == bits(want['arg'])).all()
    for k in ('half', 'host_half'):
        assert (bits(got[k]) == bits(want['half'])).all(), k
    for k in ('cone', 'cone_null', 'cone_host'):
        assert (bits(got[k]) == bits(want['cone'])).all(), k


@needs_fma
def test_cones_arg_equals_the_model_and_the_host_asin_path_on_the_fixture_worlds(vo_host):
    for i, (index, rec) in enumerate(vo_cases.fixture()):
        p = metrics._params(index)
        got = run_host(vo_host, vo_cases.fixture_agents(rec), vo_cases.positions_of(p, 120))
        assert_same(got, vo_cases.fixture_model(i, 120))


@needs_fma
def test_cones_arg_equals_the_model_and_the_host_asin_path_on_the_adversarial_world(vo_host):
    want = vo_cases.adversarial_model()
    got = run_host(vo_host, vo_cases.adversarial(), vo_cases.ADV_POS)
    assert_same(got, want)
    # the case holds what it is meant to hold: asin(1.0) exactly, and a collided position whose pairs have arg > 1 (half 0) and
    # arg <= 1 (half = asin(arg), although the cone is (0, 0))
    assert got['arg'][1, 0] == 1.0 and got['half'][1, 0] == np.pi / 2
    assert got['collided'].tolist() == [0, 0, 1]
    assert got['arg'][2, 6] > 1 and got['arg'][2, 69] > 1 and got['half'][2, 6] == 0.0 and got['half'][2, 69] == 0.0
    rest = np.delete(np.arange(70), [6, 69])
    assert (got['arg'][2, rest] <= 1).all() and (got['half'][2, rest] > 0).all() and not got['cone'][2].any()


@needs_fma
def test_cones_arg_and_asin_run_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (nothing is loaded into this process; the sanitizers' runtimes are linked into it): exactly sized heap
    arrays, the adversarial world whole, every position alone and N = 1, then d2d_asin over its cuts' neighbourhoods, every table row
    and every root seed"""
    exe = host_build.sanitized(['vo_asin_host_main.c', 'vo_asin_host.c'], tmp_path, 'vo_asin_host_main', include=CSRC)
    ag, want = vo_cases.adversarial(), vo_cases.adversarial_model()
    case = tmp_path / 'case.bin'
    with open(case, 'wb') as f:
        f.write(np.array([ag.shape[1], len(vo_cases.ADV_POS)], np.int32).tobytes())
        for a in (ag, vo_cases.ADV_POS, want['half'], want['cone']):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == ''
