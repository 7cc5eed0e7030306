"""The case table of the device world construction (include/d2d_worlds.h), shared by test_world_seq_cpu.py (the sequential host
form) and test_gpu_device_worlds.py (the kernel): every case is a list of Params, one world each, and every comparison is
array_equal against host_init.init_world for the same Params -- no tolerance anywhere."""
import ctypes as C
import os

import numpy as np

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ('agents', 'agent_unit', 'dyn_prev', 'gt', 'dmap', 'drone', 'target', 'targets', 'counters', 'active', 'kf', 'kf_len')
EXTRA = ('tracker_radius', 'obstacles', 'status')


def _seeded(pkg, ids, **kw):
    out = []
    for m in ids:
        out.append(pkg.Params(planner='NoMove', map_id=int(m), **kw))
    return out


def cases(pkg):
    """name -> (list of Params, options: grid_tile, max_attempts, capped)"""
    P = pkg.Params
    c = {}
    c['readme_b67_rng'] = (_seeded(pkg, range(1, 68), agent_number=10, agent_radius=15, agent_max_speed=20, var_cam=2), {})
    c['no_agents'] = (_seeded(pkg, range(3), agent_number=0), {})
    c['one_agent'] = (_seeded(pkg, [0], agent_number=1), {})
    c['n64'] = (_seeded(pkg, range(5), agent_number=64, agent_radius=10), {})
    c['n65'] = (_seeded(pkg, range(5), agent_number=65, agent_radius=10), {})
    c['n100_r15'] = (_seeded(pkg, [0, 1, 2, 3], agent_number=100, agent_radius=15), {})
    c['random_radius'] = (_seeded(pkg, range(8), agent_radius=-1), {})
    c['pillars'] = (_seeded(pkg, range(9), pillar_number=5, agent_number=10), {})
    c['random_map_0'] = (_seeded(pkg, range(3), agent_number=50, static_map='maps/random_map_0.npy'), {})
    c['obstacle_map'] = (_seeded(pkg, range(3), static_map='maps/obstacle_map.npy'), {})
    big = dict(map_size=[2720, 2600], agent_number=12)
    c['big_rowmajor'] = (_seeded(pkg, range(3), **big), dict(grid_tile=0))
    c['big_tiled'] = (_seeded(pkg, range(3), **big), dict(grid_tile=16))
    c['nine_settings'] = ([P(planner='NoMove', map_id=4, agent_number=10, agent_radius=r, agent_max_speed=v)
                           for r in (5, 10, 15) for v in (20, 40, 60)], {})
    c['seed_edges'] = (_seeded(pkg, [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]), {})
    c['three_targets_offset5'] = (_seeded(pkg, range(5, 9), target_list=[[50, 460], [400, 400], [450, 60]], init_pos=[250, 460]), {})
    c['cap'] = (_seeded(pkg, range(4), map_size=[200, 200], agent_number=40, agent_radius=15, init_pos=[50, 50], target_list=[[50, 160]]),
                dict(max_attempts=2000, capped=True))
    return c


CASE_NAMES = ('readme_b67_rng', 'no_agents', 'one_agent', 'n64', 'n65', 'n100_r15', 'random_radius', 'pillars', 'random_map_0',
              'obstacle_map', 'big_rowmajor', 'big_tiled', 'nine_settings', 'seed_edges', 'three_targets_offset5', 'cap')
_expected_cache = {}


def expected(pkg, name, plist, grid_tile=0):
    """host_init.init_world of every Params, stacked the way the batch stores it (computed once per case and layout)"""
    key = (name, grid_tile)
    if key in _expected_cache:
        return _expected_cache[key]
    from drone2d_amd import host_init
    from drone2d_amd.params import with_defaults
    out = stack_worlds(pkg, [host_init.init_world(with_defaults(p)) for p in plist], grid_tile)
    _expected_cache[key] = out
    return out


def stack_worlds(pkg, ws, grid_tile=0):
    """host_init.init_world dicts `ws`, stacked the way the batch stores them, read-only"""
    from drone2d_amd import state
    A = pkg._abi
    out = {}
    for f in ('agents', 'agent_unit', 'dyn_prev', 'gt', 'dmap', 'drone', 'target', 'targets', 'counters', 'tracker_radius',
              'obstacles', 'rng'):
        out[f] = np.stack([w[f] for w in ws])
    if grid_tile:
        for f in ('gt', 'dmap'):
            out[f] = state.tile_grid(out[f], grid_tile).numpy()
    B, N = len(ws), ws[0]['N']
    out['active'] = np.zeros((B, N), dtype=np.uint8)
    kf = np.zeros((B, N, A.KF))
    for i, v in ((0, 1.0), (5, 1.0), (10, 10.0), (15, 10.0)):
        kf[:, :, 4 + i] = v
    out['kf'] = kf
    out['kf_len'] = np.ones((B, N), dtype=np.int32)
    out['status'] = np.zeros(B, dtype=np.int32)
    out['group'] = ws[0]['group']
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_equal(got, exp, with_rng):
    """every world field plus tracker_radius, obstacles and status, bit for bit"""
    for f in FIELDS + EXTRA + (('rng',) if with_rng else ()):
        g, e = np.asarray(got[f]), np.asarray(exp[f])
        assert g.shape == e.shape, (f, g.shape, e.shape)
        assert g.dtype == e.dtype or f in ('obstacles', 'rng'), (f, g.dtype, e.dtype)
        assert np.array_equal(g.astype(e.dtype) if f == 'obstacles' else g.view(e.dtype) if f == 'rng' else g, e), f


def assert_capped(got):
    """an env that reached max_attempts: status set, every field 0"""
    assert (np.asarray(got['status']) == 1).all()
    for f in FIELDS + ('tracker_radius', 'obstacles'):
        assert not np.asarray(got[f]).any(), f


# ---------------------------------------------------------------------------------------- the sequential host form
def build_world_host(tmpdir):
    """gcc build of tests/csrc/world_host.c; returns (lib, run) with run(pkg, plist, grid_tile=0, max_attempts=None, rng=False) ->
    dict of numpy fields"""
    lib = host_build.shared('world_host.c', tmpdir, 'libworldhost.so')
    lib.d2d_worlds_host_build.argtypes = [C.c_void_p, C.c_void_p]
    lib.d2d_worlds_host_build.restype = C.c_int
    lib.d2d_worlds_host_python.argtypes = [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    lib.d2d_worlds_host_python.restype = None
    lib.d2d_worlds_host_numpy.argtypes = [C.c_uint32, C.c_void_p]
    lib.d2d_worlds_host_numpy.restype = None

    def run(pkg, plist, grid_tile=0, max_attempts=None, rng=False):
        from drone2d_amd import vec_env
        A = pkg._abi
        inp = vec_env.world_inputs(plist, max_attempts)
        U, N, T, P, W, H = (inp[k] for k in ('U', 'N', 'T', 'P', 'W', 'H'))
        G = (-(-W // grid_tile)) * (-(-H // grid_tile)) * grid_tile * grid_tile if grid_tile else W * H
        gshape = (U, G) if grid_tile else (U, W, H)
        i32, u8 = np.int32, np.uint8
        out = dict(agents=np.full((U, A.AF, N), 7.0), agent_unit=np.full((U, N), 7, i32), dyn_prev=np.full((U, N, 3), 7, i32),
                   gt=np.full(gshape, 7, u8), dmap=np.full(gshape, 7, u8), drone=np.full((U, A.DF), 7.0), target=np.full((U, 2), 7.0),
                   targets=np.full((U, T, 2), 7.0), counters=np.full((U, A.CF), 7, i32), active=np.full((U, N), 7, u8),
                   kf=np.full((U, N, A.KF), 7.0), kf_len=np.full((U, N), 7, i32), tracker_radius=np.full((U, N), 7.0),
                   obstacles=np.full((U, P, 3), 7, i32), status=np.full(U, 7, i32))
        if rng:
            out['rng'] = np.full((U, A.RNG_WORDS), 7, np.uint32)
        arrays = dict(inp, **out)
        spec = vec_env.world_spec(inp, grid_tile, lambda n: arrays[n].ctypes.data)
        st = A.State()
        for n in A.STATE_FIELDS:
            setattr(st, n, out[n].ctypes.data if n in out else None)
        rc = lib.d2d_worlds_host_build(C.byref(spec), C.byref(st))
        assert rc == 0
        out['group'] = inp['group']
        return out
    return lib, run
