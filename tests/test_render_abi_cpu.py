"""include/d2d_render.h and include/d2d_render_hooks.h against their ctypes binding (drone2d_amd._abi), as tests/test_gaze_abi_cpu.py
does for the gaze library."""
import ctypes as C
import os
import re

import pytest
import torch

from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_render.h')).read()
HOOKS = open(os.path.join(ROOT, 'include', 'd2d_render_hooks.h')).read()
KINDS = {'int32_t': C.c_int32, 'uint8_t': C.c_uint8, 'double': C.c_double}


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def define(name, text=TEXT):
    return int(re.search(r'#define\s+' + name + r'\s+(\w+)', text).group(1), 0)


def fields_of(struct, text):
    """[(name, ctype)] of `typedef struct <struct> { ... }` as written: pointers are c_void_p, name[n] an array"""
    body = re.search(r'typedef struct ' + struct + r' \{(.*?)\} ' + struct + ';', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip() for n in decl.split(',')]
        kind, names[0] = names[0].rsplit(None, 1)
        for n in names:
            if '*' in kind or n.startswith('*'):
                out.append((n.lstrip('*'), C.c_void_p))
                continue
            base = KINDS[kind.replace('const', '').strip()]
            m = re.match(r'(\w+)\[(\w+)\]', n)
            out.append((m.group(1), base * (define(m.group(2)) if not m.group(2).isdigit() else int(m.group(2)))) if m else (n, base))
    return out


def same(a, b):
    return [(n, C.sizeof(t), getattr(t, '_length_', 0)) for n, t in a] == [(n, C.sizeof(t), getattr(t, '_length_', 0)) for n, t in b]


def test_every_entry_point_is_bound_with_the_header_s_arguments():
    bound = A.bind_render(Recorder())
    declared = re.findall(r'^(?:int|const char \*)\s*(d2d_render_\w+)\(([^;]*)\);', TEXT + HOOKS, re.M)
    assert sorted(n for n, _ in declared) == ['d2d_render_frame', 'd2d_render_last_error', 'd2d_render_list', 'd2d_render_raster',
                                              'd2d_render_version']
    assert sorted('d2d_render_' + k for k in bound) == sorted(n for n, _ in declared)
    for name, args in declared:
        args = args.replace('\n', ' ').strip()
        want = [] if args == 'void' else [C.POINTER(A.Cfg) if 'd2d_cfg' in a else C.POINTER(A.State) if 'd2d_state' in a else
                                          C.POINTER(A.RasterCall) if 'd2d_render_raster_call' in a else
                                          C.POINTER(A.RenderCall) if 'd2d_render_call' in a else C.c_void_p for a in args.split(',')]
        fn = bound[name[len('d2d_render_'):]]
        assert fn.argtypes == want, name
        assert fn.restype is (C.c_char_p if name.endswith('last_error') else C.c_int), name
    assert 'd2d_render_raster' not in TEXT                   # the hook is declared apart from the main surface


def test_the_structs_are_the_headers_field_for_field():
    assert same(fields_of('d2d_render_item', TEXT), A.RenderItem._fields_) and C.sizeof(A.RenderItem) == A.RENDER_ITEM_BYTES == 176
    call = fields_of('d2d_render_call', TEXT)
    assert same(call, A.RenderCall._fields_)
    assert [n for n, t in call if t is C.c_void_p] == list(A.RENDER_CALL_POINTERS)
    assert [n for n, t in call if t is C.c_int32] == list(A.RENDER_CALL_INTS)
    raster = fields_of('d2d_render_raster_call', HOOKS)
    assert same(raster, A.RasterCall._fields_)
    assert [n for n, t in raster if t is C.c_void_p] == list(A.RASTER_CALL_POINTERS)


def test_version_kinds_and_limits():
    assert define('D2D_RENDER_VERSION') == A.D2D_RENDER_VERSION == 1
    assert [define('D2D_RK_' + k) for k in ('DISC', 'LINE', 'ARC', 'POLY')] == [A.RK_DISC, A.RK_LINE, A.RK_ARC, A.RK_POLY] == [1, 2, 3, 4]
    assert define('D2D_RENDER_GEOM') == A.RENDER_GEOM == 20 and define('D2D_RENDER_FIXED') == A.RENDER_FIXED == 10
    assert define('D2D_RENDER_MAX_DOWNSAMPLE') == A.RENDER_MAX_DOWNSAMPLE
    assert (define('D2D_RENDER_OK'), define('D2D_RENDER_OVERFLOW')) == (A.RENDER_OK, A.RENDER_OVERFLOW) == (0, 1)
    assert 'D2D_RENDER_FIXED + (P) + 2 * (N) + ((K) > 1 ? (K) - 1 : 0)' in TEXT
    assert A.render_cap(3, 10, 0) == 33 and A.render_cap(0, 0, 1) == 10 and A.render_cap(0, 2, 5) == 18
    import render_model as RM
    assert (RM.DISC, RM.LINE, RM.ARC, RM.POLY, RM.GEOM) == (A.RK_DISC, A.RK_LINE, A.RK_ARC, A.RK_POLY, A.RENDER_GEOM)


def test_the_library_is_registered_and_the_backend_says_so():
    assert _lib._LIBRARIES['libd2d_render.so'][0] is A.bind_render and _lib._LIBRARIES['libd2d_render.so'][2] == 'D2D_RENDER_VERSION'
    assert _lib._LIBRARIES['libd2d_render.so'][4] == 'render/build.sh'
    assert os.path.isfile(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'render', 'build.sh'))
    assert _lib.RENDER_LIB_PATH.endswith(os.path.join('csrc', 'render', 'libd2d_render.so'))
    assert _lib.HipBackend.supports_render is True and callable(_lib.load_render_library)
    assert all(callable(getattr(_lib.HipBackend, n)) for n in ('render_list', 'render_frame', 'render_raster'))
    flags = open(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'render', 'build.sh')).read()
    tracks = open(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'tracks', 'build.sh')).read()
    line = lambda s: re.search(r'\$HIPCC (.*?)\\', s).group(1)           # noqa: E731
    assert line(flags) == line(tracks) and '-ffp-contract=off' in line(flags)


def test_a_library_without_a_symbol_is_refused():
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_render_raster':
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    with pytest.raises(AttributeError):
        A.bind_render(Old())


def test_a_backend_without_the_renderer_and_the_facade_s_warning(pkg, oracle):
    """render_list() / render_frames() on a backend that has no renderer say so; Drone2DEnv2.render() keeps its warning and its None"""
    from drone2d_amd import vec_env
    env = vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', agent_number=3), 2, device='cpu', backend=oracle)
    assert tuple(env.state.pillars.shape) == (2, 0, 3)
    for call in (env.render_list, env.render_frames):
        with pytest.raises(NotImplementedError, match='has no renderer'):
            call()
    # the refusals that need no launch, on a backend that says it renders
    env.backend = type('Renders', (type(oracle),), {'supports_render': True})()
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match='downsample'):
            env.render_frames(downsample=bad)
    with pytest.raises(IndexError):
        env.render_list([0, 2])
    with pytest.raises(TypeError, match='int32 or int64'):
        env.render_list(torch.zeros(2))
    with pytest.raises(ValueError, match='out is a contiguous uint8 tensor'):
        env.render_frames(out=torch.zeros((2, 10, 10, 3), dtype=torch.uint8))
    assert tuple(env.render_frames([], downsample=4).shape) == (0, 125, 125, 3)       # S == 0: an empty tensor, no launch
    # the facade: one warning, None -- as tests/test_env_facade_cpu.py has it
    import warnings
    from drone2d_amd import env as envmod
    e = envmod.Drone2DEnv2(pkg.Params(planner='NoMove', agent_number=3), backend=oracle)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert e.render() is None and e.render('human') is None
    assert len(seen) == 1 and 'headless' in str(seen[0].message)
