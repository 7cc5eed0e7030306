"""The redraw of the validation study without a GPU: host_init.init_world(redraw=True) against the reference's recorded draws
(tests/golden/validation_episodes.npz), the scalar statement of csrc/worlds/d2d_worlds.h (d2d_w_redraw) against libm and numpy, the
sequential host form of the device build with D2D_WE_REDRAW set against init_world, a stand-alone sanitized program around both, and
the fixture's episodes on the CPU backends: their rows are the reference's."""
import ctypes as C
import math
import random
import subprocess

import numpy as np
import pytest

import host_build
import table_model as TM
import world_cases as WC

needs_fma = host_build.needs_fma('glibc dispatches its non-FMA sin / cos variant on this CPU: the restated one is the FMA variant')


def _world_params(pkg, cfg):
    return pkg.with_defaults(pkg.Params(planner='NoMove', map_id=cfg['map_id'], agent_number=cfg['agent_number'],
                                        agent_radius=cfg['agent_radius'], agent_max_speed=cfg['agent_max_speed'],
                                        static_map=cfg['static_map'], init_pos=cfg['start'], target_list=[cfg['target']]))


def _recorded(e):
    """(raw random() pairs, redrawn pref_velocity) of a fixture episode: of the played redraw, or of the world-only one"""
    return (e['pairs'], e['pref']) if e['cfg']['redraw'] else (e['x_pairs'], e['x_pref'])


def test_the_fixture_holds_what_it_is_for():
    eps, _ = TM.golden()
    forms = {(e['cfg']['form'], e['cfg']['agent_radius'], e['cfg']['agent_max_speed']) for e in eps}
    assert {('speed', 5, 40), ('speed', 15, 40), ('size', -1, 20), ('size', -1, 60)} <= forms
    assert any(e['cfg']['static_map'] == 'maps/obstacle_map.npy' and int(e['N']) > e['cfg']['agent_number'] and e['cfg']['redraw'] for e in eps)
    assert any(e['cfg']['redraw'] and int(e['py_pos']) + 4 * int(e['N']) > 624 for e in eps)          # crosses a key regeneration
    assert len({tuple(e['row'][4:9]) for e in eps}) >= 3                                                  # goal, collision, freeze, ...
    assert any('row_plain' in e and not np.array_equal(e['row'], e['row_plain'], equal_nan=True) for e in eps)
    assert all(len(_recorded(e)[0]) == int(e['N']) for e in eps)


def test_host_redraw_reproduces_the_reference(pkg):
    """bit for bit in pref_velocity; rng and every other field equal to redraw=False; the draws are those of Random(map_id) behind
    the construction"""
    from drone2d_amd import host_init
    A = pkg._abi
    eps, _ = TM.golden()
    for i, e in enumerate(eps):
        p = _world_params(pkg, e['cfg'])
        w, w0 = host_init.init_world(p, redraw=True), host_init.init_world(p)
        pairs, pref = _recorded(e)
        assert w['N'] == int(e['N'])
        assert np.array_equal(w['agents'][[A.A_VX, A.A_VY]].T, pref), i
        assert set(w) == set(w0)
        for k in w:
            if k != 'agents':
                assert np.array_equal(w[k], w0[k]), (i, k)
        assert np.array_equal(w['agents'][[A.A_PX, A.A_PY, A.A_R, A.A_R2]], w0['agents'][[A.A_PX, A.A_PY, A.A_R, A.A_R2]]), i
        assert not np.array_equal(w['agents'], w0['agents'])
        # redraw_agent_velocities on a stream of its own: the recorded raw draws give the recorded velocities

        class Replay:
            it = iter(pairs.reshape(-1).tolist())

            def random(self):
                return next(self.it)
        again = host_init.redraw_agent_velocities(dict(agents=w0['agents'].copy()), Replay())
        assert np.array_equal(again['agents'], w['agents']), i


@pytest.fixture(scope='module')
def redraw_host(tmp_path_factory):
    lib = host_build.shared('redraw_host.c', tmp_path_factory.mktemp('redraw_host'), 'libredrawhost.so')
    lib.d2d_redraw_host_words.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.d2d_redraw_host_words.restype = None
    lib.d2d_redraw_host_angles.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.d2d_redraw_host_angles.restype = None
    return lib


def _words(r):
    """the tempered words (g0, g1) of which random() makes r: r = ((g0 >> 5) * 2**26 + (g1 >> 6)) / 2**53"""
    x = (np.asarray(r, dtype=np.float64) * 2.0 ** 53).astype(np.uint64)
    return ((x >> np.uint64(26)) << np.uint64(5)).astype(np.uint32), ((x & np.uint64((1 << 26) - 1)) << np.uint64(6)).astype(np.uint32)


@needs_fma
def test_scalar_statement_against_libm(redraw_host):
    """1 048 576 arguments (r * 2.0) * pi with r from Python's random: the library's cos and sin are math.cos and math.sin, the
    contract being glibc's values; the whole statement then equals the script's three lines evaluated with math"""
    n = 1 << 20
    rnd = random.Random(20240)
    r = np.array([rnd.random() for _ in range(n)], dtype=np.float64)
    angle, c, s = (np.empty(n) for _ in range(3))
    redraw_host.d2d_redraw_host_angles(n, r.ctypes.data, angle.ctypes.data, c.ctypes.data, s.ctypes.data)
    assert angle.tolist() == [x * 2 * math.pi for x in r.tolist()]
    wc, ws = np.array([math.cos(a) for a in angle.tolist()]), np.array([math.sin(a) for a in angle.tolist()])
    for name, got, want in (('cos', c, wc), ('sin', s, ws)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, angle[bad[0]].hex(), got[bad[0]].hex(), want[bad[0]].hex())
    # the statement: agent k takes r[2 k], r[2 k + 1]
    g = np.empty(2 * n, dtype=np.uint32)
    g[0::2], g[1::2] = _words(r)
    out = np.empty(n)
    redraw_host.d2d_redraw_host_words(n // 2, g.ctypes.data, out.ctypes.data)
    vel = [x * 40 + 20 for x in r[0::2].tolist()]
    want = np.empty(n)
    want[0::2] = [v * cc for v, cc in zip(vel, wc[1::2].tolist())]
    want[1::2] = [v * ss for v, ss in zip(vel, ws[1::2].tolist())]
    assert np.array_equal(out, want)


@needs_fma
def test_scalar_statement_against_numpy_on_the_fixture(redraw_host):
    """on the reference's own draws the statement gives the reference's pref_velocity, which numpy computed; a numpy whose cos or
    sin leaves libm's values shows up here by its argument"""
    eps, _ = TM.golden()
    for i, e in enumerate(eps):
        pairs, pref = _recorded(e)
        n = len(pairs)
        g = np.empty(4 * n, dtype=np.uint32)
        g[0::4], g[1::4] = _words(pairs[:, 0])
        g[2::4], g[3::4] = _words(pairs[:, 1])
        out = np.empty(2 * n)
        redraw_host.d2d_redraw_host_words(n, g.ctypes.data, out.ctypes.data)
        angle = pairs[:, 1] * 2 * np.pi
        for k in range(n):
            assert np.cos(angle[k]) == math.cos(angle[k]) and np.sin(angle[k]) == math.sin(angle[k]), (i, k, float(angle[k]).hex())
        assert np.array_equal(np.cos(angle), [math.cos(a) for a in angle.tolist()]), i      # the array form too
        assert np.array_equal(out.reshape(n, 2), pref), i


CASES = {
    'no_agents': dict(agent_number=0),
    'n3': dict(agent_number=3),
    'n70': dict(agent_number=70, agent_radius=5),
    'n172_random_map_0': dict(agent_number=50, static_map='maps/random_map_0.npy'),
    'random_radius': dict(agent_radius=-1, agent_max_speed=20),
    'obstacle_map_pillars': dict(static_map='maps/obstacle_map.npy', pillar_number=3, agent_radius=15),
    'starts_two_targets': None,
}


def case_params(pkg, name):
    if name == 'starts_two_targets':
        return [pkg.Params(planner='NoMove', map_id=m, agent_number=10, init_pos=s, target_list=t)
                for m, s, t in ((0, [40, 40], [[250, 250], [460, 40]]), (1, [460, 250], [[40, 40], [250, 460]]), (7, [250, 460], [[460, 460], [40, 250]]))]
    return [pkg.Params(planner='NoMove', map_id=m, **CASES[name]) for m in (0, 3)]


@pytest.fixture(scope='module')
def world_host(tmp_path_factory):
    return WC.build_world_host(tmp_path_factory.mktemp('world_host_redraw'))[0]


def seq_build(pkg, lib, plist, redraw, grid_tile=0):
    """world_cases.build_world_host's run() with the redraw handed to world_inputs"""
    from drone2d_amd import vec_env
    A = pkg._abi
    inp = vec_env.world_inputs(plist, redraw=redraw)
    U, N, T, P, W, H = (inp[k] for k in ('U', 'N', 'T', 'P', 'W', 'H'))
    i32, u8 = np.int32, np.uint8
    out = dict(agents=np.full((U, A.AF, N), 7.0), agent_unit=np.full((U, N), 7, i32), dyn_prev=np.full((U, N, 3), 7, i32),
               gt=np.full((U, W, H), 7, u8), dmap=np.full((U, W, H), 7, u8), drone=np.full((U, A.DF), 7.0), target=np.full((U, 2), 7.0),
               targets=np.full((U, T, 2), 7.0), counters=np.full((U, A.CF), 7, i32), active=np.full((U, N), 7, u8),
               kf=np.full((U, N, A.KF), 7.0), kf_len=np.full((U, N), 7, i32), tracker_radius=np.full((U, N), 7.0),
               obstacles=np.full((U, P, 3), 7, i32), status=np.full(U, 7, i32), rng=np.full((U, A.RNG_WORDS), 7, np.uint32))
    arrays = dict(inp, **out)
    spec = vec_env.world_spec(inp, grid_tile, lambda n: arrays[n].ctypes.data)
    st = A.State()
    for n in A.STATE_FIELDS:
        setattr(st, n, out[n].ctypes.data if n in out else None)
    assert lib.d2d_worlds_host_build(C.byref(spec), C.byref(st)) == 0
    return out


@needs_fma
@pytest.mark.parametrize('name', list(CASES))
def test_sequential_build_with_the_redraw_is_init_world(pkg, world_host, name):
    from drone2d_amd import host_init
    plist = case_params(pkg, name)
    for redraw in (True, False):
        got = seq_build(pkg, world_host, plist, redraw)
        exp = WC.stack_worlds(pkg, [host_init.init_world(pkg.with_defaults(p), redraw=redraw) for p in plist])
        WC.assert_equal(got, exp, with_rng=True)
    if name == 'n172_random_map_0':
        assert got['agents'].shape[2] == 172


def test_sanitized_program_around_the_host_built_header(tmp_path):
    """AddressSanitizer and UBSan on the scalar statement and the sequential build with the redraw, in a program of its own"""
    exe = host_build.sanitized(['redraw_host_main.c'], tmp_path, 'redraw_host_main')
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    st = out.stdout.split()
    assert st[:3] == ['0', '0', '0'] and math.isfinite(float(st[3]))


def test_fixture_rows_on_the_cpu_backends(pkg):
    """The fixture's episodes from host worlds with the redraw, through the closed loop of the oracle (the 'speed' form: Primitive /
    Oxford) and through the step path's episode loop (the 'size' form: Jerk_Primitive / NoControl): the rows are the reference's.
    Without the redraw the rows of the 'speed' form are the reference's rows without it, which differ: the parent of this change
    cannot produce the first."""
    eps, tie = TM.golden()
    differs = 0
    for idx, plist, redraw, speed in TM.golden_cells(pkg):
        rows = TM.rows_of_worlds(plist[0], plist, redraw, speed, jerk_tie=tie)
        for i, r in zip(idx, rows):
            c = eps[i]['cfg']
            assert TM.same_numbers(r, eps[i]['row']), (i, TM.row_numbers(r).tolist(), eps[i]['row'].tolist())
            assert r[:12] == (plist[0].gaze_method, plist[0].planner, 'CVM', c['map_id'], c['agent_radius'], c['agent_number'], 0,
                              -1 if redraw else c['agent_max_speed'], c['drone_max_speed'], 0, tuple(c['start']), tuple(c['target']))
        if redraw and any('row_plain' in eps[i] for i in idx):
            plain = TM.rows_of_worlds(plist[0], plist, False, speed)
            for i, r in zip(idx, plain):
                if 'row_plain' in eps[i]:
                    assert TM.same_numbers(r, eps[i]['row_plain']), i
                    differs += not TM.same_numbers(r, eps[i]['row'])
    assert differs >= 1


def test_reset_restores_the_redrawn_world(pkg, oracle):
    """the snapshot is taken behind the redraw: reset() gives what the script's env.reset() and redraw give"""
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', map_id=3, agent_number=6)
    env = vec_env.VecDrone2DEnv(p, 2, device='cpu', backend=oracle, redraw_agents=True)
    want = np.stack([w['agents'] for w in vec_env.build_worlds(p, 2, redraw=True)])
    assert np.array_equal(env.state.agents.numpy(), want)
    assert not np.array_equal(want, np.stack([w['agents'] for w in vec_env.build_worlds(p, 2)]))
    for _ in range(5):
        env.step(0.5)
    assert not np.array_equal(env.state.agents.numpy(), want)
    env.reset()
    assert np.array_equal(env.state.agents.numpy(), want)
