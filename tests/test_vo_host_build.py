"""csrc/metrics/d2d_vo.h (the arithmetic of the velocity-obstacle kernels) compiled for the host with gcc, against the Python model
bit for bit: every intermediate and every count.  A second, stand-alone build of the same loops runs under AddressSanitizer and
UBSan as a program of its own.  test_gpu_vo_metric.py checks the device build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vo_cases
from drone2d_amd import _abi as A
from drone2d_amd import metrics
import host_build

CSRC = os.path.join(host_build.CSRC, 'metrics')
needs_fma = host_build.needs_fma('libm dispatches non-FMA sin / cos / atan2 variants on this CPU')


@pytest.fixture(scope='module')
def vo_host(tmp_path_factory):
    lib = host_build.shared('vo_host.c', tmp_path_factory.mktemp('vo'), 'libvohost.so', include=CSRC)
    V, I = C.c_void_p, C.c_int32
    lib.vo_host_geometry.argtypes = [V, V, C.c_double, I, I, I, V, V, V]
    lib.vo_host_cones.argtypes = [V, V, V, I, I, I, V]
    lib.vo_host_count.argtypes = [V, V, V, V, I, I, I, I, V]
    return lib


def run_host(lib, agents, pos, cand, rA=5.0):
    """agents [B, 6, N] -> the dict vo_model.vo_world returns, with a leading B"""
    agents, pos, cand = (np.ascontiguousarray(a, np.float64) for a in (agents, pos, cand))
    B, _, N = agents.shape
    P, Cn = len(pos), len(cand)
    arg, tba = np.full((B, P, N), np.nan), np.full((B, P, N), np.nan)
    col = np.full((B, P), 0x7f, np.uint8)
    cone = np.full((B, P, N, 2), np.nan)
    count = np.full((B, P), 0x7f7f7f7f, np.int32)
    lib.vo_host_geometry(agents.ctypes.data, pos.ctypes.data, rA, B, N, P, arg.ctypes.data, tba.ctypes.data, col.ctypes.data)
    half = metrics.host_asin(arg)
    lib.vo_host_cones(tba.ctypes.data, half.ctypes.data, col.ctypes.data, B, N, P, cone.ctypes.data)
    lib.vo_host_count(agents.ctypes.data, cand.ctypes.data, cone.ctypes.data, col.ctypes.data, B, N, P, Cn, count.ctypes.data)
    return dict(count=count, collided=col, arg=arg, theta_ba=tba, half=half, cone=cone)


def assert_same(got, want, b=0):
    for k in ('collided', 'count'):
        assert np.array_equal(got[k][b], want[k]), k
    for k in ('arg', 'theta_ba', 'half', 'cone'):
        g, w = np.ascontiguousarray(got[k][b]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and (g.view(np.int64) == w.view(np.int64)).all(), k


@needs_fma
def test_host_build_equals_the_model_on_the_fixture_worlds(vo_host):
    fx = vo_cases.fixture()
    for i, (index, rec) in enumerate(fx):
        p = metrics._params(index)
        got = run_host(vo_host, vo_cases.fixture_agents(rec)[None], vo_cases.positions_of(p, 120), vo_cases.candidates())
        assert_same(got, vo_cases.fixture_model(i, 120))


@needs_fma
def test_host_build_equals_the_model_on_the_adversarial_world(vo_host):
    want = vo_cases.adversarial_model()
    got = run_host(vo_host, vo_cases.adversarial()[None], vo_cases.ADV_POS, vo_cases.candidates())
    assert_same(got, want)
    # the case holds what it is meant to hold
    assert want['count'].tolist()[2] == -1 and want['collided'].tolist() == [0, 0, 1]
    assert want['arg'][1, 0] == 1.0 and want['half'][1, 0] == np.pi / 2
    assert want['theta_ba'][1, 1] == np.pi
    r, l = want['cone'][1, 1]
    assert abs(r - l) > 3.14 and l < 0 < r                        # first wrap branch
    r, l = want['cone'][1, 2]
    assert abs(r - l) > 3.14 and r < 0 < l                        # second wrap branch
    assert want['arg'][2, 6] > 1 and want['arg'][2, 69] > 1


def test_header_version_is_the_binding_s(vo_host):
    vo_host.vo_host_version.restype = C.c_int
    assert vo_host.vo_host_version() == A.D2D_METRICS_VERSION


@needs_fma
def test_host_loops_run_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (nothing is loaded into this process; the sanitizers' runtimes are linked into it): exactly sized heap
    arrays, the adversarial world whole and cut down to C = 1, C = 65, P = 1 and N = 1"""
    exe = host_build.sanitized(['vo_host_main.c', 'vo_host.c'], tmp_path, 'vo_host_main', include=CSRC)
    ag, cand, want = vo_cases.adversarial(), vo_cases.candidates(), vo_cases.adversarial_model()
    case = tmp_path / 'case.bin'
    with open(case, 'wb') as f:
        f.write(np.array([ag.shape[1], len(vo_cases.ADV_POS), len(cand)], np.int32).tobytes())
        for a in (ag, vo_cases.ADV_POS, cand):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(want['count'].astype(np.int32).tobytes())
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == ''
