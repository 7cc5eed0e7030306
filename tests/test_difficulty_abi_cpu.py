"""include/d2d_metrics.h against its ctypes binding (drone2d_amd._abi) for the traversability and survival-fit entry points."""
import ctypes as C
import os
import re

from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_metrics.h')).read()


def define(name):
    return eval(re.search(r'#define\s+' + name + r'\s+(.+?)\s*(/\*|$)', TEXT, re.M).group(1))


def test_version_and_limits_equal_the_header():
    assert define('D2D_METRICS_VERSION') == A.D2D_METRICS_VERSION >= 2
    assert define('D2D_TRAV_MAX_ELEMS') == A.TRAV_MAX_ELEMS
    assert (define('D2D_FIT_MAX_N'), define('D2D_FIT_MAX_P'), define('D2D_FIT_MAX_ELEMS')) == (A.FIT_MAX_N, A.FIT_MAX_P, A.FIT_MAX_ELEMS)


def test_the_two_symbols_are_declared_and_bound_with_the_header_s_arguments():
    kinds = {'int32_t': C.c_int32, 'double': C.c_double}

    class Lib:
        def __getattr__(self, name):
            fn = type('fn', (), {})()
            self.__dict__[name] = fn
            return fn
    bound = A.bind_metrics(Lib())
    for name in ('d2d_trav_steps', 'd2d_fit_first_hit'):
        m = re.search(r'\bint ' + name + r'\(([^;]*)\);', TEXT)
        assert m, name
        want = [C.c_void_p if '*' in arg else kinds[arg.split()[0]] for arg in m.group(1).replace('\n', ' ').split(',')]
        fn = bound[name.replace('d2d_', '')]
        assert fn.restype is C.c_int and fn.argtypes == want, name
    assert _lib.HipBackend.supports_difficulty_tables is True and _lib.HipBackend.supports_vo_metric is True
    assert callable(_lib.HipBackend.trav_steps) and callable(_lib.HipBackend.fit_first_hit)
