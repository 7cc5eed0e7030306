"""include/d2d_jerk_live.h against its ctypes binding (drone2d_amd._abi.bind_jerk_live): the addition to libd2d_jerk.so that leaves
finished envs alone, bound as an optional symbol next to the pinned surface of include/d2d_jerk.h."""
import ctypes as C
import os
import re

from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = open(os.path.join(ROOT, 'include', 'd2d_jerk_live.h')).read()
JERK = open(os.path.join(ROOT, 'include', 'd2d_jerk.h')).read()
D2D = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
DECL = r'^(?:int|const char \*)\s*(d2d_\w+)\(([^;]*)\);'


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def argtypes_of(args):
    return [C.POINTER(A.JerkCall) if 'd2d_jerk_call' in a else C.c_void_p for a in args.replace('\n', ' ').split(',') if '*' in a]


def test_the_header_against_both_binders():
    declared = dict(re.findall(DECL, LIVE, re.M))
    assert sorted(declared) == ['d2d_jerk_plan_live']
    live, pinned = A.bind_jerk_live(Recorder()), A.bind_jerk(Recorder())
    assert sorted('d2d_jerk_' + k for k in live) == sorted(declared) == sorted('d2d_jerk_' + k for k in A.JERK_LIVE_ENTRY_POINTS)
    assert not set(live) & set(pinned) and sorted(pinned) == ['last_error', 'plan', 'reset', 'version']     # still exactly four names
    fn = live['plan_live']
    args = declared['d2d_jerk_plan_live']
    assert len(args.split(',')) == 3 and fn.argtypes == argtypes_of(args) == [C.POINTER(A.JerkCall), C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    # the arguments of the unmasked function with `flags` put in after the call
    unmasked = dict(re.findall(DECL, JERK, re.M))['d2d_jerk_plan']
    assert fn.argtypes[:1] + fn.argtypes[2:] == argtypes_of(unmasked) == pinned['plan'].argtypes
    names = [a.replace('*', ' ').split()[-1] for a in args.replace('\n', ' ').split(',')]
    assert names == ['call', 'flags', 'stream']


def test_the_done_byte_and_the_library_s_version():
    define = lambda text, n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', text).group(1), 0)   # noqa: E731
    assert define(LIVE, 'D2D_JERK_LIVE_F_DONE') == define(D2D, 'D2D_F_DONE') == A.F_DONE == A.JERK_LIVE_F_DONE == 3
    assert '#define D2D_JERK_VERSION' not in LIVE and define(JERK, 'D2D_JERK_VERSION') == A.D2D_JERK_VERSION == 1
    assert re.findall(r'#include "(d2d[^"]*)"', LIVE) == ['d2d_jerk.h']     # the call's struct; include/d2d.h is not needed
    assert _lib._LIBRARIES['libd2d_jerk.so'][0] is A.bind_jerk          # the live function is bound on the same loaded library
    assert callable(_lib.HipBackend.jerk_plan_live) and hasattr(_lib.HipBackend, 'supports_jerk_live')


def test_a_library_without_the_live_symbol_binds_nothing_and_the_flag_is_false():
    class Old(Recorder):
        def __getattr__(self, name):
            if name.endswith('_live'):
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    assert A.bind_jerk_live(Old()) == {} and sorted(A.bind_jerk(Old())) == ['last_error', 'plan', 'reset', 'version']
    hip = object.__new__(_lib.HipBackend)                               # no GPU: the flag only looks at what was bound
    hip.jlib, hip.jfn = Old(), A.bind_jerk(Old())
    assert hip.supports_jerk_live is False
    hip.jfn = dict(hip.jfn, **A.bind_jerk_live(Recorder()))
    assert hip.supports_jerk_live is True


def test_the_built_library_exports_it_and_refuses_bad_arguments_without_a_gpu(pkg):
    """bad arguments are refused before any launch, so this runs without a GPU"""
    lib, jfn = _lib.load_jerk_library()
    live = A.bind_jerk_live(lib)
    assert sorted(live) == ['plan_live'] and jfn['version']() == 1
    one = C.c_void_p(8)                      # never dereferenced: every call below is refused first
    c = A.JerkCall()
    for k in A.JERK_CALL_POINTERS:
        setattr(c, k, 8)
    c.B, c.N, c.S, c.W, c.H, c.grid_tile, c.scale, c.W_px, c.H_px = 2, 3, 9, 50, 50, 0, 10.0, 500.0, 500.0
    err = lambda: jfn['last_error']().decode()                                                  # noqa: E731
    assert live['plan_live'](C.byref(c), None, None) == -1
    assert err() == 'd2d_jerk_plan_live: flags is NULL (d2d_jerk_plan is the launch without a mask)'
    assert live['plan_live'](None, one, None) == -1 and 'call is NULL' in err()
    for field, value, rc, text in (('S', A.JERK_MAX_S + 1, -4, 'samples a primitive'), ('N', A.JERK_MAX_N + 1, -4, 'trackers'),
                                   ('B', 0, -1, 'B >= 1'), ('grid_tile', 8, -1, 'grid_tile'), ('tie_perm', None, -1, 'table pointer is NULL'),
                                   ('wp', None, -1, 'output pointer is NULL'), ('trk_prev', None, -1, 'tracker pointer is NULL')):
        keep = getattr(c, field)
        setattr(c, field, value)
        assert live['plan_live'](C.byref(c), one, None) == rc and text in err() and err().startswith('d2d_jerk_plan_live: '), field
        got = err()[len('d2d_jerk_plan_live: '):]
        assert jfn['plan'](C.byref(c), None) == rc and err() == 'd2d_jerk_plan: ' + got, field     # d2d_jerk_plan's own refusal
        setattr(c, field, keep)
