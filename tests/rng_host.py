"""Host build of csrc/d2d_rng.h (tests/csrc/rng_host.c) and the numpy side of the comparisons: shared by test_rng_cpu.py and the
GPU tests of the device noise stream."""
import ctypes as C
import platform

import numpy as np
import pytest

import host_build

RNG_WORDS, RNG_POS, RNG_NPAIR, RNG_NREGEN = 640, 624, 625, 626

# the stream calls libm's log through csrc/d2d_log.h: the same two conditions as tests/test_log.py
needs_glibc_235 = pytest.mark.skipif(platform.libc_ver()[0] != 'glibc' or platform.libc_ver()[1] != '2.35',
                                     reason=f'd2d_log.h restates the log of glibc 2.35; this host has {platform.libc_ver()}')
needs_fma = host_build.needs_fma('libm dispatches a non-FMA log variant on this CPU')


def build_rng_host(tmpdir):
    """draw(state uint32[640], m) -> float64 [m, 2]; advances `state` in place"""
    lib = host_build.shared('rng_host.c', tmpdir, 'librnghost.so')
    lib.d2d_rng_host_draw.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.d2d_rng_host_draw.restype = C.c_int

    def draw(state, m):
        assert state.dtype == np.uint32 and state.shape == (RNG_WORDS,) and state.flags.c_contiguous
        out = np.empty((m, 2), dtype=np.float64)
        assert lib.d2d_rng_host_draw(state.ctypes.data, m, out.ctypes.data) == m
        return out
    return draw


def numpy_stream(state):
    """A RandomState at the stream `state` (uint32[640]: key, position; the Gaussian cache is empty)"""
    rs = np.random.RandomState()
    rs.set_state(('MT19937', state[:624].copy(), int(state[RNG_POS]), 0, 0.0))
    return rs


def numpy_pairs(rs, m):
    """what utils.py:605 draws for m agents in view, in agent order: [m, 2]"""
    return np.array([rs.randn(2) for _ in range(m)], dtype=np.float64).reshape(m, 2)


def assert_state_is(state, rs, what=''):
    """`state` against RandomState.get_state(): the position always; the key too -- numpy regenerates lazily, at the first draw
    that needs a word (position 624 with the old key), where the restatements regenerate just as lazily, so the keys agree too"""
    _, key, pos, has_gauss, _ = rs.get_state()
    assert has_gauss == 0, what
    assert int(state[RNG_POS]) == pos, (what, int(state[RNG_POS]), pos)
    assert np.array_equal(state[:624], key), what
    assert not state[RNG_NREGEN + 1:].any(), what
