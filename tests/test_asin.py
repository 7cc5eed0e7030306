"""csrc/metrics/d2d_asin.h (the asin of the velocity-obstacle cones) compiled for the host, against libm's asin bit for bit, and
against math.asin on a sample.  test_gpu_asin.py checks the device build.  Expected values come from libm through a C helper and
from math.asin, never from np.arcsin (numpy may dispatch its own vectorised asin)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import asin_cases
import host_build

CSRC = os.path.join(host_build.CSRC, 'metrics')
TABLE = os.path.join(CSRC, 'd2d_asin_tbl.h')
TOOL = os.path.join(host_build.ROOT, 'tools', 'extract_asin_table.py')


@pytest.fixture(scope='module')
def asin_host(tmp_path_factory):
    """(restatement, libm) as numpy functions of x"""
    lib = host_build.shared('asin_host.c', tmp_path_factory.mktemp('asin'), 'libasinhost.so', include=CSRC)

    def wrap(f):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]

        def call(x):
            x = np.ascontiguousarray(x, np.float64)
            out = np.empty_like(x)
            f(x.ctypes.data, out.ctypes.data, x.size)
            return out
        return call
    return wrap(lib.d2d_asin_host_array), wrap(lib.d2d_asin_libm_array)


def asin_args(seed=11):
    """1.9e7 arguments over every branch of the restatement, its cuts and the metric's own quotients"""
    rng = np.random.RandomState(seed)
    n = 1_000_000
    sign = rng.choice([-1.0, 1.0], n)
    return np.concatenate([asin_cases.per_branch(rng, n), asin_cases.cut_neighbourhoods(2000), sign * 10.0 ** rng.uniform(-320, 0, n),
                           asin_cases.vo_shaped(rng, n), rng.uniform(-1, 1, n), asin_cases.SPECIALS])


@host_build.needs_fma('libm dispatches a non-FMA asin variant on this CPU')
def test_asin_restatement_is_bit_identical_to_libm(asin_host):
    mine, libm = asin_host
    x = asin_args()
    assert x.size >= 10_000_000
    got = mine(x)
    bad = np.flatnonzero(~asin_cases.same_bits(got, libm(x)))
    assert bad.size == 0, [(x[i].hex(), got[i].hex()) for i in bad[:8]]
    # the helper's expected values are Python's math.asin: on a sample, on the cuts and on every special case
    idx = np.r_[np.random.RandomState(3).randint(0, x.size, 200_000), np.arange(x.size - asin_cases.SPECIALS.size, x.size)]
    assert asin_cases.same_bits(got[idx], asin_cases.math_asin(x[idx])).all()
    w = asin_cases.cut_neighbourhoods(50)
    assert asin_cases.same_bits(mine(w), asin_cases.math_asin(w)).all()


def test_asin_special_values(asin_host):
    mine, _ = asin_host
    got = mine(asin_cases.SPECIALS)
    hp = float.fromhex('0x1.921fb54442d18p+0')
    assert got[0] == 0.0 and not np.signbit(got[0]) and got[1] == 0.0 and np.signbit(got[1])
    assert got[2] == hp and got[3] == -hp
    assert np.isnan(got[4:9]).all() and np.isnan(got[-4:]).all()
    assert asin_cases.same_bits(got[9:15], asin_cases.SPECIALS[9:15]).all()       # subnormals and the smallest normal: asin x = x


def test_committed_table_is_what_the_tool_extracts(tmp_path):
    sys.path.insert(0, os.path.dirname(TOOL))
    try:
        import extract_asin_table
    finally:
        sys.path.pop(0)
    if extract_asin_table.tables() is None:
        pytest.skip('this libm does not hold glibc 2.35\'s asincos.tbl / root.tbl')
    out = tmp_path / 'd2d_asin_tbl.h'
    subprocess.check_call([sys.executable, TOOL, str(out)])
    assert out.read_bytes() == open(TABLE, 'rb').read()
