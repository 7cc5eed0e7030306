"""The sequential host form of the device world construction (csrc/worlds/d2d_worlds.h, built by tests/csrc/world_host.c) against
host_init.init_world: the case table of world_cases.py and the 20 configurations of tests/golden/init_cases.npz, every field bit
for bit; and the two random streams alone against Python's `random` and numpy's RandomState."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import world_cases as WC
from replay import load
from rng_host import needs_fma, needs_glibc_235


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return WC.build_world_host(tmp_path_factory.mktemp('worldhost'))


def test_streams_match_python_and_numpy(host):
    """No libm anywhere: the seeded key, 300 random() (one regeneration) and 40 _randbelow(401) against random.Random, the kept
    numpy state against RandomState(seed) after rand(100), for 200 seeds with the edge values among them."""
    lib, _ = host
    seeds = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + [int(s) for s in np.random.RandomState(7).randint(0, 2 ** 32, 194, dtype=np.uint64)]
    nd, nr, n = 330, 40, 401
    key, d, r, st = np.zeros(624, np.uint32), np.zeros(nd), np.zeros(nr, np.uint32), np.zeros(640, np.uint32)
    for s in seeds:
        lib.d2d_worlds_host_python(s, key.ctypes.data, nd, d.ctypes.data, nr, n, r.ctypes.data)
        rnd = random.Random(s)
        state = rnd.getstate()[1]
        assert state[624] == 624 and np.array_equal(key, np.array(state[:624], dtype=np.uint32)), s
        assert d.tolist() == [rnd.random() for _ in range(nd)], s
        assert r.tolist() == [rnd.randint(50, 450) - 50 for _ in range(nr)], s
        lib.d2d_worlds_host_numpy(s, st.ctypes.data)
        rs = np.random.RandomState(s)
        rs.rand(100)
        _, k, pos, has_gauss, _ = rs.get_state()
        assert pos == 200 == st[624] and has_gauss == 0 and np.array_equal(st[:624], k) and not st[625:].any(), s


def test_map_id_outside_numpys_seeds_is_refused(pkg):
    from drone2d_amd import vec_env
    for bad in (2 ** 32, -1):
        with pytest.raises(ValueError, match='map_id'):
            vec_env.world_inputs([pkg.Params(map_id=bad)])
        with pytest.raises(ValueError):
            np.random.RandomState(bad)


def test_n_t_and_group_are_known_before_anything_is_built(pkg):
    from drone2d_amd import host_init, vec_env
    p = pkg.Params(agent_number=50, static_map='maps/random_map_0.npy', target_list=[[50, 460], [400, 400]])
    inp = vec_env.world_inputs([p])
    w = host_init.init_world(p)
    assert (inp['N'], inp['T']) == (w['N'], w['T']) == (172, 2)
    assert np.array_equal(inp['group'], w['group'])


def test_cpu_backend_has_no_device_worlds(pkg, oracle):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', agent_number=3)
    with pytest.raises(NotImplementedError, match='device world'):
        vec_env.VecDrone2DEnv(p, 2, backend=oracle, worlds='device')
    with pytest.raises(NotImplementedError, match='device world'):
        vec_env.build_worlds_device(p, 2, backend=oracle)


@needs_glibc_235
@needs_fma
@pytest.mark.parametrize('name', WC.CASE_NAMES)
def test_case_table(pkg, host, name):
    plist, opt = WC.cases(pkg)[name]
    tile = opt.get('grid_tile', 0)
    with_rng = any(p.var_cam != 0 for p in plist)
    got = host[1](pkg, plist, grid_tile=tile, max_attempts=opt.get('max_attempts'), rng=with_rng)
    if opt.get('capped'):
        WC.assert_capped(got)
        return
    exp = WC.expected(pkg, name, plist, tile)
    WC.assert_equal(got, exp, with_rng)
    assert np.array_equal(got['group'], exp['group'])


@needs_glibc_235
@needs_fma
def test_init_cases_of_the_reference(pkg, host):
    """the 20 configurations captured from the reference (the fixture that pins host_init itself)"""
    fx = load('init_cases')
    A = pkg._abi
    for i in range(int(fx['n_cfg'])):
        cfg = json.loads(str(fx[f'c{i}_cfg']))
        p = pkg.Params(planner='NoMove', **cfg)
        got = host[1](pkg, [p], rng=True)
        exp = WC.expected(pkg, f'init{i}', [p])
        WC.assert_equal(got, exp, True)
        ag = got['agents'][0]
        assert np.array_equal(ag[A.A_PX], fx[f'c{i}_agent_pos'][:, 0]) and np.array_equal(ag[A.A_PY], fx[f'c{i}_agent_pos'][:, 1])
        assert np.array_equal(ag[A.A_VX], fx[f'c{i}_agent_pref'][:, 0]) and np.array_equal(ag[A.A_VY], fx[f'c{i}_agent_pref'][:, 1])
        assert np.array_equal(ag[A.A_R], fx[f'c{i}_agent_radius'])
        assert np.array_equal(got['obstacles'][0], fx[f'c{i}_obstacles'])
        assert np.array_equal(got["gt"][0], fx[f'c{i}_gt0'])


def test_header_is_plain_c_and_matches_the_ctypes_mirror(pkg, tmp_path):
    """include/d2d_worlds.h compiles as C99 and as C++, and d2d_world_spec has the size and the constants of _abi.WorldSpec"""
    import os
    import shutil
    import subprocess
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    A = pkg._abi
    src = tmp_path / 'hdr.c'
    src.write_text('#include "include/d2d_worlds.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) { printf("%zu %zu %zu %d %d %d %d\\n", sizeof(d2d_world_spec), offsetof(d2d_world_spec, start_clear), '
                   'offsetof(d2d_world_spec, unit), D2D_WORLDS_VERSION, D2D_WORLDS_ENV_F, D2D_WORLDS_MAX_ATTEMPTS, D2D_WE_NTGT); return 0; }\n')
    exe = tmp_path / 'hdr'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', WC.ROOT, str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(A.WorldSpec), A.WorldSpec.start_clear.offset, A.WorldSpec.unit.offset, A.D2D_WORLDS_VERSION,
                   A.WORLDS_ENV_F, A.WORLDS_MAX_ATTEMPTS, A.WE_NTGT]
    subprocess.check_call(['g++', '-std=c++11', '-Wall', '-Werror', '-I', WC.ROOT, '-x', 'c++', '-fsyntax-only', str(src)])


def test_library_checks_the_spec_without_a_gpu(pkg):
    """libd2d_worlds.so loads on a CPU-only box, reports its version and refuses a bad spec before any launch"""
    from drone2d_amd import _lib, vec_env
    A = pkg._abi
    _, fn = _lib.load_worlds_library()
    assert fn['version']() == A.D2D_WORLDS_VERSION
    inp = vec_env.world_inputs([pkg.Params(agent_number=10, pillar_number=5)], map_ids=range(1, 5))
    assert inp['U'] == 4 and inp['env_par'].shape == (4, A.WORLDS_ENV_F) and inp['map_id'].tolist() == [1, 2, 3, 4]
    spec = vec_env.world_spec(inp, 0, lambda n: None)
    out = (C.c_int32 * 2)()
    assert fn['launch_shape'](C.byref(spec), C.byref(out)) == 0 and tuple(out) == (1, 32 * 10 + 4 * 632 + 12 * 5)
    spec.version += 1
    assert fn['launch_shape'](C.byref(spec), C.byref(out)) == -2 and b'version' in fn['last_error']()
    spec.version -= 1
    st = A.State()
    assert fn['build'](C.byref(spec), C.byref(st), None) == -1 and b'NULL' in fn['last_error']()      # no array behind the spec
    spec.grid_tile = 8
    assert fn['launch_shape'](C.byref(spec), C.byref(out)) == -1
    spec.grid_tile, spec.max_attempts = 0, 0
    assert fn['launch_shape'](C.byref(spec), C.byref(out)) == -1
