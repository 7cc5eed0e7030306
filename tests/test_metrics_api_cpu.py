"""The Python surface of the difficulty metrics (drone2d_amd.metrics) where it needs no GPU: positions, candidates, density,
table order, the backend gate and the ABI constants."""
import math
import os
import re

import numpy as np
import pytest

import vo_cases
from drone2d_amd import _abi as A
from drone2d_amd import metrics, sweeps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_positions_are_the_script_s_ranges():
    index, _ = vo_cases.fixture()[0]
    p = metrics._params(index)
    xs, ys = metrics.vo_positions(p)
    assert xs == ys == list(range(10, 490, 30)) and len(xs) * len(ys) == 256
    p.map_size = [500, 300]
    xs, ys = metrics.vo_positions(p, 120)
    assert xs == [10, 130, 250, 370] and ys == [10, 130, 250]
    pos = vo_cases.positions_of(p, 120)
    assert pos.shape == (12, 2) and pos[:4].tolist() == [[10, 10], [10, 130], [10, 250], [130, 10]]      # x outermost


def test_candidates_are_the_script_s_expressions():
    cand = metrics.vo_candidates()
    assert cand.shape == (630, 2) and cand.dtype == np.float64
    assert cand[0].tolist() == [20.0, 0.0]
    th = float(np.arange(0, 2 * 3.14, 0.1)[62])
    assert cand[629].tolist() == [56.0 * math.cos(th), 56.0 * math.sin(th)]
    assert cand[13].tolist() == [32.0 * math.cos(0.1), 32.0 * math.sin(0.1)]            # theta outermost, 10 speeds each
    assert (cand[629, 0].hex(), cand[629, 1].hex()) == ((56.0 * math.cos(th)).hex(), (56.0 * math.sin(th)).hex())
    assert metrics.vo_candidates(10, 30).shape == (630, 2) and metrics.vo_candidates(10, 30)[1, 0] == 12.0


@pytest.mark.parametrize('i', range(3))
def test_density_equals_the_recorded_reference(i):
    index, rec = vo_cases.fixture()[i]
    got = metrics.density(index)
    assert isinstance(got, float) and got.hex() == float(rec['density']).hex()
    with pytest.raises(NotImplementedError, match='density_calculator.py'):
        metrics.density(dict(index, agent_size=-1))


def test_tables_follow_the_script_s_loop_order(monkeypatch):
    args = ([3, 1], (20, 10), (5, 15), (20, 60))
    order = sweeps._table_order(*args)
    seen = []

    def fake_batch(indices, position_step=30, device='cuda:0', backend=None, worlds=None, timings=None):
        assert len({ix['agent_number'] for ix in indices}) == 1          # a batch shares N
        seen.extend(indices)
        return np.array([[order.index(ix), order.index(ix)] for ix in indices], dtype=np.float64)
    monkeypatch.setattr(metrics, 'vo_feasibility_batch', fake_batch)
    t = metrics.vo_table(*args)
    assert len(t) == 2 and all(len(row) == 8 for row in t)
    assert [v for row in t for v in row] == list(range(16))
    assert sorted(map(order.index, seen)) == list(range(16))
    monkeypatch.setattr(metrics, 'density', lambda ix, world=None: order.index(ix))
    d = metrics.density_table(*args)
    assert [v for row in d for v in row] == list(range(16)) and len(d) == 2
    with pytest.raises(ValueError):
        metrics.vo_table(*args, worlds=[None] * 3)


def test_density_table_on_real_worlds():
    index, rec = vo_cases.fixture()[0]
    t = metrics.density_table([index['map_id']], (index['agent_number'],), (index['agent_size'],), (index['agent_speed'],))
    assert t == [[float(rec['density'])]]


def test_a_backend_without_the_library_is_refused(oracle):
    index, _ = vo_cases.fixture()[0]
    for call in (lambda: metrics.vo_feasibility(index, backend=oracle), lambda: metrics.vo_feasibility_batch([index], backend=oracle),
                 lambda: metrics.vo_table([0], (10,), (5,), (20,), backend=oracle)):
        with pytest.raises(NotImplementedError, match='vo_calculator.py'):
            call()
    import torch
    z = torch.zeros((1, 6, 1), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match='vo_calculator.py'):
        metrics.vo_counts(z, torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 2), dtype=torch.float64), backend=oracle)


def test_abi_constants_equal_the_header():
    text = open(os.path.join(ROOT, 'include', 'd2d_metrics.h')).read()

    def define(name):
        return eval(re.search(r'#define\s+' + name + r'\s+(.+?)\s*(/\*|$)', text, re.M).group(1))
    assert define('D2D_METRICS_VERSION') == A.D2D_METRICS_VERSION
    assert (define('D2D_VO_MAX_B'), define('D2D_VO_MAX_P'), define('D2D_VO_MAX_ELEMS')) == (A.VO_MAX_B, A.VO_MAX_P, A.VO_MAX_ELEMS)
    for fn in ('d2d_metrics_version', 'd2d_metrics_last_error', 'd2d_vo_geometry', 'd2d_vo_cones', 'd2d_vo_count'):
        assert re.search(r'\b' + fn + r'\(', text), fn


def test_the_library_is_loaded_on_first_use_only():
    """HipBackend() must work in a tree without libd2d_metrics.so: its constructor never touches the file"""
    import inspect
    from drone2d_amd import _lib
    assert 'load_metrics_library' not in inspect.getsource(_lib.HipBackend.__init__)
    with pytest.raises(_lib.D2DError, match='csrc/metrics/build.sh'):
        _lib.load_metrics_library(os.path.join(ROOT, 'no_such_dir', 'libd2d_metrics.so'))
