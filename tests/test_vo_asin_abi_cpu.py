"""include/d2d_metrics.h against its ctypes binding (drone2d_amd._abi) for the device asin's two entry points, the asin= keyword's
refusal, and the kernel-source hash the bench's PMC figures were taken on (the asin headers live outside the hashed set)."""
import ctypes as C
import json
import os
import re
import sys

import pytest

from drone2d_amd import _abi as A
from drone2d_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_metrics.h')).read()


def test_the_two_symbols_are_declared_and_bound_with_the_header_s_arguments():
    kinds = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}

    class Lib:
        def __getattr__(self, name):
            fn = type('fn', (), {})()
            self.__dict__[name] = fn
            return fn
    bound = A.bind_metrics(Lib())
    for name, nargs in (('d2d_asin_array', 4), ('d2d_vo_cones_arg', 9)):
        m = re.search(r'\bint ' + name + r'\(([^;]*)\);', TEXT)
        assert m, name
        want = [C.c_void_p if '*' in arg else kinds[arg.split()[0]] for arg in m.group(1).replace('\n', ' ').split(',')]
        fn = bound[name.replace('d2d_', '')]
        assert len(want) == nargs and fn.restype is C.c_int and fn.argtypes == want, name
    assert callable(_lib.HipBackend.asin_array) and callable(_lib.HipBackend.vo_cones_arg) and callable(metrics.device_asin)


def test_a_library_without_the_symbols_is_refused():
    class Old:
        """a libd2d_metrics.so of the same version from before the two entry points"""
        def __getattr__(self, name):
            if name in ('d2d_asin_array', 'd2d_vo_cones_arg'):
                raise AttributeError(name)
            fn = type('fn', (), {})()
            self.__dict__[name] = fn
            return fn
    with pytest.raises(AttributeError):
        A.bind_metrics(Old())


def test_the_version_stays_2_in_both_places():
    assert re.search(r'#define\s+D2D_METRICS_VERSION\s+2\b', TEXT) and A.D2D_METRICS_VERSION == 2


def test_an_unknown_asin_path_is_refused_before_any_backend_call():
    class Backend:
        """every attribute access is a failure: the keyword is checked first"""
        def __getattr__(self, name):
            raise AssertionError('backend touched: ' + name)
    for call in (lambda: metrics.vo_counts(None, None, None, backend=Backend(), asin='nonsense'),
                 lambda: metrics.vo_feasibility_batch([], backend=Backend(), asin='nonsense'),
                 lambda: metrics.vo_feasibility({}, backend=Backend(), asin=None),
                 lambda: metrics.vo_table(backend=Backend(), asin='Device')):
        with pytest.raises(ValueError, match='asin='):
            call()
    assert metrics.ASIN_PATHS == ('device', 'host') and callable(metrics.host_asin)


def test_the_kernel_source_hash_is_the_profiles():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import src_hash
    finally:
        sys.path.pop(0)
    stored = json.load(open(os.path.join(ROOT, 'profiles', 'pmc_latest.json')))
    recs = [v for v in stored.values() if isinstance(v, dict) and 'shape' in v]
    for m in stored.get('more', []):
        recs += [v for v in m.values() if isinstance(v, dict)]
    assert recs and {v.get('src_hash') for v in recs} == {src_hash.source_hash()}
