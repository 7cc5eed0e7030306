"""csrc/metrics/d2d_difficulty.h (the arithmetic of the traversability and survival-fit kernels) compiled for the host with gcc,
against the Python model: step counts, first hits and final agents, bit for bit.  A second, stand-alone build of the same loops
runs under AddressSanitizer and UBSan as a program of its own.  test_gpu_difficulty_tables.py checks the device build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import difficulty_cases as DC
import difficulty_model as M
from drone2d_amd import _abi as A
from drone2d_amd import sweeps
import host_build

CSRC = os.path.join(host_build.CSRC, 'metrics')
needs_fma = host_build.needs_fma('numpy takes non-FMA norm / matmul variants on this CPU')


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    lib = host_build.shared('difficulty_host.c', tmp_path_factory.mktemp('difficulty'), 'libdifficultyhost.so', include=CSRC)
    V, I, D = C.c_void_p, C.c_int32, C.c_double
    lib.difficulty_host_trav_steps.argtypes = [V, I, I, I, V, I, V]
    lib.difficulty_host_fit_first_hit.argtypes = [V, V, D, D, D, D, D, I, I, I, I, V, V, V]
    return lib


def host_steps(lib, grids, starts):
    grids = np.ascontiguousarray(grids, np.uint8)
    st = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
    B, W, H = grids.shape
    out = np.full((B, len(st), 8), 0x7f7f7f7f, np.int32)
    lib.difficulty_host_trav_steps(grids.ctypes.data, B, W, H, st.ctypes.data, len(st), out.ctypes.data)
    return out


def host_fit(lib, agents, pos, checks, drone_radius=10.0, map_size=(500, 500), scale=10, dt=0.1, want_agents=True):
    agents, pos = np.ascontiguousarray(agents, np.float64), np.ascontiguousarray(pos, np.float64)
    B, _, N = agents.shape
    first = np.full((B, len(pos)), 0x7f7f7f7f, np.int32)
    end = np.full(agents.shape, np.nan) if want_agents else None
    work = np.zeros(5 * N)
    lib.difficulty_host_fit_first_hit(agents.ctypes.data, pos.ctypes.data, drone_radius, map_size[0], map_size[1], scale, dt, B, N, len(pos),
                                      checks, first.ctypes.data, None if end is None else end.ctypes.data, work.ctypes.data)
    return first, end


def test_walks_equal_the_model(host):
    got = host_steps(host, np.stack([rec['gt'] for _, rec in DC.fixture()]), DC.AXIS_STARTS)
    for i in range(5):
        assert np.array_equal(got[i], DC.fixture_trav_model(i)['steps'])
    assert np.array_equal(host_steps(host, DC.small_grid()[None], DC.SMALL_STARTS)[0], DC.grid_model('small'))
    args = (300, 260, 33, 5)
    grid, starts = DC.GRIDS['random'](*args)
    assert np.array_equal(host_steps(host, grid[None], starts)[0], DC.grid_model('random', *args))


@needs_fma
def test_first_hits_and_final_agents_equal_the_model_on_the_fixture_worlds(host):
    for i, (index, rec) in enumerate(DC.fixture()):
        p = sweeps._params(index)
        first, end = host_fit(host, rec['fit_agents'][None], DC.positions_of(p), DC.CHECKS, p.drone_radius, p.map_size, p.map_scale, p.dt)
        m = DC.fixture_fit_model(i)
        assert np.array_equal(first[0], m['first'])
        assert DC.bits_equal(end[0], m['agents_end']) and DC.bits_equal(end[0], rec['fit_agents_end'])
        assert DC.bits_equal(M.fit_times(first[0], (8, 8)), rec['survive_times'])


@needs_fma
@pytest.mark.parametrize('N', [1, 24, 70])
def test_first_hits_and_final_agents_equal_the_model_on_the_adversarial_world(host, N):
    for kw in (dict(), dict(touching=True), dict(drone_radius=0), dict(P=65, checks=1)):
        ag, m = DC.adversarial_fit_model(N, **kw)
        first, end = host_fit(host, ag[None], DC.fit_positions(kw.get('P', 64)), kw.get('checks', DC.CHECKS), kw.get('drone_radius', 10))
        assert np.array_equal(first[0], m['first']), kw
        assert DC.bits_equal(end[0], m['agents_end']), kw
    two = np.stack([DC.adversarial_fit_model(N)[0], DC.adversarial_fit_model(N, roll=1)[0]])
    first, end = host_fit(host, two, DC.fit_positions(64), DC.CHECKS, want_agents=False)
    assert end is None and np.array_equal(first[1], DC.adversarial_fit_model(N, roll=1)[1]['first'])


def test_header_version_is_the_binding_s(host):
    host.difficulty_host_version.restype = C.c_int
    assert host.difficulty_host_version() == A.D2D_METRICS_VERSION >= 2


@needs_fma
def test_host_loops_run_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (nothing is loaded into this process; the sanitizers' runtimes are linked into it): exactly sized heap
    arrays, the 7 x 5 grid and the adversarial world whole and cut down to S = 1, P = 1, N = 1, no check and no agents_out"""
    exe = host_build.sanitized(['difficulty_host_main.c', 'difficulty_host.c'], tmp_path, 'difficulty_host_main', include=CSRC)
    grid, steps = DC.small_grid(), DC.grid_model('small')
    ag, m = DC.adversarial_fit_model(70, P=65)
    pos = DC.fit_positions(65)
    case = tmp_path / 'case.bin'
    with open(case, 'wb') as f:
        f.write(np.array([grid.shape[0], grid.shape[1], len(DC.SMALL_STARTS), ag.shape[1], len(pos), DC.CHECKS], np.int32).tobytes())
        f.write(np.ascontiguousarray(grid, np.uint8).tobytes())
        f.write(np.array(DC.SMALL_STARTS, np.int32).tobytes())
        f.write(np.ascontiguousarray(steps, np.int32).tobytes())
        f.write(np.ascontiguousarray(ag, np.float64).tobytes())
        f.write(np.ascontiguousarray(pos, np.float64).tobytes())
        f.write(np.ascontiguousarray(m['first'], np.int32).tobytes())
        f.write(np.ascontiguousarray(m['agents_end'], np.float64).tobytes())
    r = subprocess.run([exe, str(case)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == ''
