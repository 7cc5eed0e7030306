"""The device build of csrc/metrics/d2d_asin.h through its test hook d2d_asin_array (drone2d_amd.metrics.device_asin), against
Python's math.asin bit for bit: every branch in both signs, the neighbourhoods of the cuts and the special values, NaN written by
hand where math.asin raises (|x| > 1) and for NaN.  test_asin.py checks the host build of the same text on > 10^7 arguments."""
import functools

import numpy as np
import pytest
import torch

import asin_cases
from drone2d_amd import _lib, metrics

pytestmark = pytest.mark.gpu
G = 64


@functools.lru_cache(maxsize=None)
def case():
    """(x, math.asin(x)): 1e5 arguments per branch and sign, the cuts' neighbourhoods, the metric's own quotients and the specials,
    in a fixed random order so that every prefix holds every branch"""
    rng = np.random.RandomState(5)
    x = np.concatenate([asin_cases.per_branch(rng, 100_000), asin_cases.cut_neighbourhoods(2000), asin_cases.vo_shaped(rng, 20_000),
                        asin_cases.SPECIALS])
    x = x[rng.permutation(x.size)]
    x.setflags(write=False)
    want = asin_cases.math_asin(x)
    want.setflags(write=False)
    return x, want


def on(hip, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(hip.device)


def test_every_branch_cut_and_special_value_equals_math_asin(hip):
    x, want = case()
    assert x.size > 1_600_000 and np.isnan(want).sum() >= 7
    got = metrics.device_asin(on(hip, x), backend=hip).cpu().numpy()
    bad = np.flatnonzero(~asin_cases.same_bits(got, want))
    assert bad.size == 0, [(x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]
    sp = metrics.device_asin(on(hip, asin_cases.SPECIALS), backend=hip).cpu().numpy()      # ... and the special values in their order
    assert asin_cases.same_bits(sp, asin_cases.math_asin(asin_cases.SPECIALS)).all()
    assert np.signbit(sp[1]) and not np.signbit(sp[0]) and sp[2] == np.pi / 2 and sp[3] == -np.pi / 2


@pytest.mark.parametrize('n', [1, 65, 2 ** 20 + 3])
def test_sizes_with_a_partial_last_workgroup_write_exactly_inside(hip, n):
    x, want = case()
    raw = torch.full(((n + 2 * G) * 8,), 0x7f, dtype=torch.uint8, device=hip.device)
    whole = raw.view(torch.float64)
    out = whole[G:G + n]
    hip.asin_array(on(hip, x[:n]), out)
    hip.sync()
    assert asin_cases.same_bits(out.cpu().numpy(), want[:n]).all()
    guard = torch.cat([whole[:G], whole[-G:]]).contiguous().view(torch.uint8)
    assert bool((guard == 0x7f).all())


def test_out_may_alias_x(hip):
    x, want = case()
    n = 100_002
    t = on(hip, x[:n])
    hip.asin_array(t, t)
    hip.sync()
    assert asin_cases.same_bits(t.cpu().numpy(), want[:n]).all()
    v = on(hip, x[:n]).reshape(7, -1)[:, :100]                      # device_asin of a view: a new tensor of its shape
    got = metrics.device_asin(v, backend=hip)
    assert got.shape == v.shape and asin_cases.same_bits(got.cpu().numpy().ravel(), want[:n].reshape(7, -1)[:, :100].ravel()).all()
    with pytest.raises(ValueError):
        metrics.device_asin(v.float(), backend=hip)


def test_n_0_launches_nothing_and_bad_arguments_are_refused(hip):
    out = torch.full((8,), 0x7f, dtype=torch.uint8, device=hip.device).repeat(8).view(torch.float64)
    before = out.clone()
    p = out.data_ptr()
    hip._metrics('asin_array', p, 0, p)                               # returns 0: no D2DError
    hip.sync()
    assert torch.equal(out.view(torch.int64), before.view(torch.int64))
    assert metrics.device_asin(torch.empty((0,), dtype=torch.float64, device=hip.device), backend=hip).numel() == 0
    for args in ((p, -1, p), (None, 8, p), (p, 8, None), (None, 0, None)):
        with pytest.raises(_lib.D2DError, match='error -1:'):
            hip._metrics('asin_array', *args)
    hip.sync()
    assert torch.equal(out.view(torch.int64), before.view(torch.int64))
