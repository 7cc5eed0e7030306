"""include/d2d_rvo_live.h and include/d2d_stepped.h against their ctypes bindings (drone2d_amd._abi): the additions to libd2d_rvo.so
and libd2d_hip.so that leave finished envs alone, bound as optional symbols next to the pinned surfaces of include/d2d_rvo.h and
include/d2d.h."""
import ctypes as C
import os
import re

import pytest

from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = open(os.path.join(ROOT, 'include', 'd2d_rvo_live.h')).read()
RVO = open(os.path.join(ROOT, 'include', 'd2d_rvo.h')).read()
STEPPED = open(os.path.join(ROOT, 'include', 'd2d_stepped.h')).read()
D2D = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
DECL = r'^(?:int|const char \*)\s*(d2d_\w+)\(([^;]*)\);'
KINDS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def argtypes_of(args, structs=None):
    out = []
    for a in args.replace('\n', ' ').strip().split(','):
        words = a.replace('*', ' * ').split()
        if '*' in words:
            struct = (structs or {}).get(words[1] if words[0] == 'const' else words[0])
            out.append(C.POINTER(struct) if struct else C.c_void_p)
        else:
            out.append(KINDS[words[0]])
    return out


def test_the_rvo_live_header_against_both_binders():
    declared = dict(re.findall(DECL, LIVE, re.M))
    assert sorted(declared) == ['d2d_rvo_agents_step_live', 'd2d_rvo_velocity_live']
    live, pinned = A.bind_rvo_live(Recorder()), A.bind_rvo(Recorder())
    assert sorted('d2d_rvo_' + k for k in live) == sorted(declared) == sorted('d2d_rvo_' + k for k in A.RVO_LIVE_ENTRY_POINTS)
    assert not set(live) & set(pinned) and sorted(pinned) == ['agents_step', 'last_error', 'velocity', 'version']
    for name, args in declared.items():
        fn = live[name[len('d2d_rvo_'):]]
        assert fn.argtypes == argtypes_of(args), name
        assert fn.restype is C.c_int, name
    # the arguments of the unmasked function with `flags` put in: after pillars, after vel
    unmasked = {n: argtypes_of(a) for n, a in re.findall(DECL, RVO, re.M) if n in ('d2d_rvo_velocity', 'd2d_rvo_agents_step')}
    v, s = list(live['velocity_live'].argtypes), list(live['agents_step_live'].argtypes)
    assert len(v) == 9 and len(s) == 10
    assert v[:3] + v[4:] == unmasked['d2d_rvo_velocity'] and v[3] is C.c_void_p
    assert s[:2] + s[3:] == unmasked['d2d_rvo_agents_step'] and s[2] is C.c_void_p
    names = lambda args: [a.replace('*', ' ').split()[-1] for a in args.replace('\n', ' ').split(',')]   # noqa: E731
    assert names(declared['d2d_rvo_velocity_live']) == ['agents', 'vel', 'pillars', 'flags', 'B', 'N', 'P', 'vel_out', 'stream']
    assert names(declared['d2d_rvo_agents_step_live']) == ['agents', 'vel', 'flags', 'W_px', 'H_px', 'scale', 'dt', 'B', 'N', 'stream']


def test_the_done_byte_and_the_library_s_version():
    define = lambda text, n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', text).group(1), 0)   # noqa: E731
    assert define(LIVE, 'D2D_RVO_LIVE_F_DONE') == define(D2D, 'D2D_F_DONE') == A.F_DONE == A.RVO_LIVE_F_DONE == 3
    assert 'D2D_RVO_VERSION' not in LIVE and define(RVO, 'D2D_RVO_VERSION') == A.D2D_RVO_VERSION == 1
    assert '#include "d2d' not in LIVE                                  # the header stands alone
    assert _lib._LIBRARIES['libd2d_rvo.so'][0] is A.bind_rvo            # the live functions are bound on the same loaded library
    assert _lib.HipBackend.supports_rvo_live is True
    assert callable(_lib.HipBackend.rvo_velocity_live) and callable(_lib.HipBackend.rvo_agents_step_live)


def test_a_library_without_the_live_symbols_binds_none_of_them():
    class Old(Recorder):
        def __getattr__(self, name):
            if name.endswith('_live'):
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    assert A.bind_rvo_live(Old()) == {} and sorted(A.bind_rvo(Old())) == ['agents_step', 'last_error', 'velocity', 'version']
    bound = A.bind(Old())
    assert 'gaze_stage' in bound and not set(A.STEPPED_ENTRY_POINTS) & set(bound)


def test_the_stepped_header_against_the_binder():
    declared = dict(re.findall(DECL, STEPPED, re.M))
    assert sorted(declared) == sorted('d2d_' + n for n in A.STEPPED_ENTRY_POINTS) == ['d2d_gaze_stage_live', 'd2d_plan_stage_live']
    bound = A.bind(Recorder())
    structs = {'d2d_cfg': A.Cfg, 'd2d_state': A.State, 'd2d_plan': A.Plan}
    for name, args in declared.items():
        fn = bound[name[len('d2d_'):]]
        assert fn.argtypes == argtypes_of(args, structs) == bound[name[len('d2d_'):-len('_live')]].argtypes, name
        assert fn.restype is C.c_int
    # additions: optional symbols, outside the surface the oracle mirrors and outside the test hooks; no version moves
    assert set(A.STEPPED_ENTRY_POINTS) <= set(A.OPTIONAL)
    assert not set(A.STEPPED_ENTRY_POINTS) & (set(A.ENTRY_POINTS) | set(A.HIP_ONLY_ENTRY_POINTS))
    assert A.D2D_ABI_VERSION == 8 and 'D2D_ABI_VERSION' not in STEPPED
    assert _lib.HipBackend.supports_stepped_plugins is True
    assert callable(_lib.HipBackend.gaze_stage_live) and callable(_lib.HipBackend.plan_stage_live)


def test_the_built_libraries_export_them_and_refuse_bad_arguments_without_a_gpu(pkg):
    """bad arguments are refused before any launch, so this runs without a GPU"""
    _, fn = _lib.load_library()
    assert set(A.STEPPED_ENTRY_POINTS) <= set(fn)
    c, s = A.Cfg(), A.State()
    for name in A.STEPPED_ENTRY_POINTS:
        assert fn[name](C.byref(c), C.byref(s), None, None) == -2 and b'ABI' in fn['last_error']()
    lib, rfn = _lib.load_rvo_library()
    live = A.bind_rvo_live(lib)
    assert sorted(live) == sorted(A.RVO_LIVE_ENTRY_POINTS) and rfn['version']() == 1
    one = C.c_void_p(8)                      # never dereferenced: every call below is refused first
    assert live['velocity_live'](one, one, None, None, 2, 3, 0, one, None) == -1 and b'flags is NULL' in rfn['last_error']()
    assert live['agents_step_live'](one, one, None, 500.0, 500.0, 10.0, 0.1, 2, 3, None) == -1 and b'flags is NULL' in rfn['last_error']()
    assert live['velocity_live'](one, one, None, one, 0, 3, 0, one, None) == -1 and b'B >= 1' in rfn['last_error']()
    assert live['velocity_live'](one, one, one, one, 2, 1000, 100, one, None) == -4 and b'cones' in rfn['last_error']()
    assert live['velocity_live'](one, one, None, one, 2, 3, 0, None, None) == -1 and b'pointer is NULL' in rfn['last_error']()
    assert live['velocity_live'](one, one, None, one, 2, 3, 0, one, None) == -1 and b'must not be vel' in rfn['last_error']()
    assert live['velocity_live'](one, one, None, one, 2, 3, 2, one, None) == -1 and b'pointer is NULL' in rfn['last_error']()
    assert live['agents_step_live'](None, one, one, 500.0, 500.0, 10.0, 0.1, 2, 3, None) == -1 and b'pointer is NULL' in rfn['last_error']()
    assert live['velocity_live'](None, None, None, one, 2, 0, 0, None, None) == 0          # N == 0: nothing to do
    assert live['agents_step_live'](None, None, one, 500.0, 500.0, 10.0, 0.1, 2, 0, None) == 0
