"""csrc/jerk/d2d_jerk.h (the arithmetic of the Jerk_Primitive kernel) compiled for the host with gcc, against the Python model: the
`_seq` loop on seeded synthetic batches, bit for bit, and the scalar pieces on their own.  A second, stand-alone build of the same
loop runs under AddressSanitizer and UBSan as a program of its own.  test_gpu_jerk.py checks the device build."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from drone2d_amd import _abi as A
from drone2d_amd import jerk_plugin as JP
import host_build
import jerk_cases as JC
import jerk_model as M

CSRC = os.path.join(host_build.CSRC, 'jerk')
needs_fma = host_build.needs_fma('numpy takes non-FMA norm variants on this CPU')
HOST_B = 64          # envs of a batch the host loop runs: nine of every kind (the device test runs 257)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    lib = host_build.shared('jerk_host.c', tmp_path_factory.mktemp('jerk'), 'libjerkhost.so', include=CSRC)
    V, I, D = C.c_void_p, C.c_int32, C.c_double
    lib.jerk_host_plan.argtypes = [C.POINTER(A.JerkCall), V]
    lib.jerk_host_reset.argtypes = [V, V, V, V, I, I, I]
    for name, args in (('mod360', [D]), ('phi', [D, D, D, D]), ('cost', [I, D])):
        getattr(lib, 'jerk_host_' + name).argtypes = args
        getattr(lib, 'jerk_host_' + name).restype = D
    lib.jerk_host_pattern.argtypes = [D]
    return lib


def run_host(lib, b):
    arr = JC.host_arrays(b)
    call = JC.call_of(b, lambda a: a.ctypes.data, arr)
    work = np.zeros(5 * max(b['N'], 1))
    assert lib.jerk_host_plan(C.byref(call), work.ctypes.data) == 0
    return arr


@needs_fma
@pytest.mark.parametrize('B,N,v_max,W,H,tile', JC.BATCHES, ids=lambda v: str(v))
def test_host_loop_equals_the_model_on_synthetic_batches(host, B, N, v_max, W, H, tile):
    b, want = JC.batch(HOST_B, N, v_max, W, H, tile), JC.answers(HOST_B, N, v_max, W, H, tile)
    got = run_host(host, b)
    assert not want['unknown'].any()                                   # the inputs hold no tie pattern outside the table
    assert np.array_equal(got['plan_ok'], want['plan_ok']) and np.array_equal(got['wp_valid'], want['plan_ok'])
    assert np.array_equal(got['choice'], want['choice'])
    assert M.bits_equal(got['wp'], want['wp'])
    assert np.array_equal(got['stat'] & A.JERK_STAT_TIE != 0, want['tie'])
    assert not (got['stat'] & A.JERK_STAT_UNKNOWN).any()
    assert np.array_equal(got['stat'] >> A.JERK_STAT_SHIFT, want['tested'])
    if N:
        assert M.bits_equal(got['trk_radius'], b['radius_after']) and np.array_equal(got['trk_prev'], b['prev_after'])
    # what the batch is for: plans that fail, ties that decide, headings rejected
    kinds = np.array(b['kinds'])
    assert (want['plan_ok'][kinds == 'blocked'] == 0).all() and want['plan_ok'][kinds == 'open'].any()
    assert want['tie'][kinds == 'wall'].any() and want['tie'][kinds == 'on_pf'].any()
    assert (want['tested'][kinds == 'on_pf'] >= 2).all()               # the best heading's samples are NaN
    if N >= 3:
        assert want['tie'][kinds == 'axis'].any() and (want['tested'][kinds == 'axis'] >= 2).all()


@needs_fma
def test_var_cam_enters_the_tracker_limit(host):
    b, want = JC.batch(HOST_B, 3, 20, 50, 50, 0, seed=1), JC.answers(HOST_B, 3, 20, 50, 50, 0, seed=1)
    assert b['var_cam'] == 2.0
    got = run_host(host, b)
    assert np.array_equal(got['choice'], want['choice']) and M.bits_equal(got['wp'], want['wp'])


def test_scalar_pieces_equal_python(host):
    rng = np.random.RandomState(5)
    for a in list(rng.uniform(-720, 720, 20000)) + [0.0, -0.0, 360.0, -360.0, 180.0, -180.0, -1e-300, 719.9999999999999, 1e15]:
        assert M.bits_equal(host.jerk_host_mod360(a), a % 360.0), a
    for _ in range(20000):
        px, py, gx, gy = rng.randint(0, 500, 4).astype(float)
        assert M.bits_equal(host.jerk_host_phi(px, py, gx, gy), math.degrees(math.atan2(gy - py, gx - px)))
    for phi in list(rng.uniform(-180, 180, 300)) + [0.0, 90.0, -90.0, 180.0, 45.0, -135.0, 2.5, 12.5, 357.5, -2.5]:
        want = JP.heading_costs(phi)
        assert M.bits_equal([host.jerk_host_cost(i, phi % 360) for i in range(72)], want), phi
        assert M.bits_equal(want, M.costs(phi))
        assert host.jerk_host_pattern(phi % 360) == JP.pattern_of(phi)
    assert host.jerk_host_pattern(float('nan')) == 0 and host.jerk_host_pattern(360.0) == 0


def test_a_table_row_that_does_not_fit_falls_back_to_cost_index_order(host):
    """a tie table recorded elsewhere whose rows are not this pattern's: (cost, index) order, and bit 1 only where a tie exists"""
    b = JC.batch(HOST_B, 0, 40, 50, 50, 0)
    arr = JC.host_arrays(b)
    arr['tie_perm'][:] = np.arange(72, dtype=np.uint8)[::-1]
    arr['tie_eq'][:] = 0
    call = JC.call_of(b, lambda a: a.ctypes.data, arr)
    work = np.zeros(5)
    assert host.jerk_host_plan(C.byref(call), work.ctypes.data) == 0
    for e in range(HOST_B):
        sc = JC.scene_of(b, e)
        cost = M.costs(M.goal_direction(sc))
        r = M.plan(sc, order=np.argsort(cost, kind='stable'))
        assert arr['choice'][e] == r['choice'] and M.bits_equal(arr['wp'][e], r['wp'])
        srt = np.sort(cost)
        assert bool(arr['stat'][e] & A.JERK_STAT_UNKNOWN) == bool((srt[1:] == srt[:-1]).any())
    arr['tie_perm'][:] = 200                                           # bytes that are no heading: never used as an index
    assert host.jerk_host_plan(C.byref(call), work.ctypes.data) == 0


def test_reset_with_a_mask(host):
    rng = np.random.RandomState(3)
    r0, r, prev = rng.uniform(5, 15, (6, 4)), rng.uniform(5, 15, (6, 4)), np.ones((6, 4), np.uint8)
    mask = np.array([[1, 9], [0, 9], [0, 9], [1, 9], [0, 9], [1, 9]], np.uint8)        # stride 2
    before = r.copy()
    host.jerk_host_reset(r.ctypes.data, prev.ctypes.data, r0.ctypes.data, mask.ctypes.data, 2, 6, 4)
    on = mask[:, 0].astype(bool)
    assert M.bits_equal(r[on], r0[on]) and M.bits_equal(r[~on], before[~on])
    assert not prev[on].any() and prev[~on].all()


def test_limits_and_version_are_the_header_s(host):
    assert host.jerk_host_version() == A.D2D_JERK_VERSION
    assert host.jerk_host_call_bytes() == C.sizeof(A.JerkCall)
    b = JC.batch(HOST_B, 0, 40, 50, 50, 0)
    arr = JC.host_arrays(b)
    call = JC.call_of(b, lambda a: a.ctypes.data, arr)
    call.S = A.JERK_MAX_S + 1
    assert host.jerk_host_plan(C.byref(call), None) == -4
    call.S, call.N = 9, A.JERK_MAX_N + 1
    assert host.jerk_host_plan(C.byref(call), None) == -4


@needs_fma
def test_host_loop_runs_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (nothing is loaded into this process; the sanitizers' runtimes are linked into it): exactly sized heap
    arrays, every synthetic batch of the model comparison above"""
    exe = host_build.sanitized(['jerk_host_main.c', 'jerk_host.c'], tmp_path, 'jerk_host_main', include=CSRC)
    case = tmp_path / 'case.bin'
    with open(case, 'wb') as f:
        f.write(np.array([len(JC.BATCHES)], np.int32).tobytes())
        for B, N, v_max, W, H, tile in JC.BATCHES:
            b, want = JC.batch(HOST_B, N, v_max, W, H, tile), JC.answers(HOST_B, N, v_max, W, H, tile)
            arr = JC.host_arrays(b)
            f.write(np.array([HOST_B, N, arr['tt_tab'].shape[1], W, H, tile, arr['dmap'].shape[1]], np.int32).tobytes())
            f.write(np.array([JC.SCALE, W * JC.SCALE, H * JC.SCALE, JC.DRONE_RADIUS, JC.AGENT_RADIUS, b['var_cam'], 0.5 * v_max]).tobytes())
            for k in ('drone', 'target', 'active', 'kf', 'dmap', 'trk_radius', 'trk_prev', 'th_tab', 'tt_tab', 'tie_perm', 'tie_eq'):
                if arr[k] is not None:
                    f.write(arr[k].tobytes())
            f.write(want['plan_ok'].tobytes())
            f.write(want['wp'].tobytes())
            f.write(want['choice'].tobytes())
            f.write(b['radius_after'].tobytes())
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == ''
