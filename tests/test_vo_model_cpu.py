"""The velocity-obstacle metric's Python model (tests/vo_model.py) against the reference's own env_metrics, recorded in
tests/golden/vo_feasibility.npz by tests/golden/make_vo_golden.py: per-position rates and their mean, bit for bit."""
import numpy as np
import pytest

import vo_cases
import vo_model
from drone2d_amd import metrics


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


@pytest.mark.parametrize('i', range(3))
def test_model_equals_the_recorded_reference(i):
    index, rec = vo_cases.fixture()[i]
    m = vo_cases.fixture_model(i, 30)
    assert len(m['count']) == 256
    rates = vo_model.rates_of(m['count'], len(vo_cases.candidates()))
    assert np.array_equal(m['collided'].astype(bool), rec['collided'])
    assert same_bits(rates, rec['rates'])
    assert same_bits(np.mean(rates), rec['mean'])


def test_fixture_covers_collisions_wraps_and_empty_positions():
    got = []
    for i, (index, rec) in enumerate(vo_cases.fixture()):
        m = vo_cases.fixture_model(i, 30)
        got.append((int(rec['collided'].sum()), vo_model.wrap_cones(m['cone'], m['collided']), int((m['count'] == 0).sum())))
    assert [g[0] for g in got] == [3, 17, 39], got
    assert all(g[1] > 50 for g in got), got
    assert got[2][2] > 0, got


@pytest.mark.parametrize('i', range(3))
def test_host_world_is_the_recorded_world(i):
    """metrics._params builds the reference's world for this script: drone_radius=0 (the survivability sweep's 10 gives others)"""
    index, rec = vo_cases.fixture()[i]
    p = metrics._params(index)
    assert p.drone_radius == 0
    w = vo_cases.world_of(p)
    assert same_bits(w['agents'], vo_cases.fixture_agents(rec))
    m = vo_model.vo_world(w['agents'], vo_cases.positions_of(p, 120), vo_cases.candidates())
    sel = [16 * (4 * a) + 4 * b for a in range(4) for b in range(4)]       # the step-120 positions inside the step-30 grid
    assert same_bits(vo_model.rates_of(m['count'], 630), rec['rates'][sel])
