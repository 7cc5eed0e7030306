"""Every text the Python plumbing of the three device libraries shows a user, against a recording (tests/golden/refusal_texts.json,
written by tests/golden/make_refusal_texts.py from the package as it was before its loaders, binders, backend gates and table
drivers were each stated once): the refusals of a backend without the kernels, of a bad `worlds` argument and of a wrong number of
worlds, what the loaders say about a missing or mismatched library, and the key sets of the metric batches' `timings`.  Everything
runs on the host: the oracle backend, the model backend of test_difficulty_model_cpu.py and the built libraries; no GPU is opened."""
import contextlib
import json
import os

import pytest
import torch

import difficulty_cases as DC
from test_difficulty_model_cpu import ModelBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'refusal_texts.json')
ONE = ([0], (10,), (5,), (20,))            # a table of one setting


class VoModelBackend(ModelBackend):
    """passes the velocity-obstacle gate too; the recorded refusals come before its first launch"""
    supports_vo_metric = True


@contextlib.contextmanager
def _patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def _refusal(call):
    try:
        call()
    except Exception as e:
        return [type(e).__name__, str(e).replace(ROOT, '<root>')]
    raise AssertionError('the call was not refused')


def record(pkg, oracle):
    from drone2d_amd import _abi as A, _lib, metrics, sweeps, vec_env
    index = DC.fixture()[0][0]
    model, vo_model = ModelBackend(), VoModelBackend()
    p = pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1)
    z = torch.zeros((1, 6, 1), dtype=torch.float64)
    xy = torch.zeros((1, 2), dtype=torch.float64)
    calls = {
        # a backend without the kernels
        'no kernels: vo_feasibility_batch': lambda: metrics.vo_feasibility_batch([index], backend=oracle),
        'no kernels: vo_counts': lambda: metrics.vo_counts(z, xy, xy, backend=oracle),
        'no kernels: traversibility_batch': lambda: metrics.traversibility_batch([index], backend=oracle),
        'no kernels: survival_fit_batch': lambda: metrics.survival_fit_batch([index], backend=oracle),
        'no kernels: trav_steps': lambda: metrics.trav_steps(torch.full((1, 7, 5), 2, dtype=torch.uint8), [(0, 0)], backend=oracle),
        'no kernels: fit_first_hit': lambda: metrics.fit_first_hit(z, xy, p, 1, backend=oracle),
        'no kernels: build_worlds_device_of': lambda: vec_env.build_worlds_device_of([p], backend=oracle),
        "no kernels: VecDrone2DEnv(worlds='device')": lambda: vec_env.VecDrone2DEnv(p, 2, backend=oracle, worlds='device'),
        "no kernels: survivability_batch(worlds='device')": lambda: sweeps.survivability_batch([index], backend=oracle, worlds='device'),
        # worlds that are neither a list nor 'device'
        'elsewhere: vo_feasibility_batch': lambda: metrics.vo_feasibility_batch([index], backend=vo_model, worlds='elsewhere'),
        'elsewhere: traversibility_batch': lambda: metrics.traversibility_batch([index], backend=model, worlds='elsewhere'),
        'elsewhere: survival_fit_batch': lambda: metrics.survival_fit_batch([index], backend=model, worlds='elsewhere'),
        'elsewhere: survivability_batch': lambda: sweeps.survivability_batch([index], backend=oracle, worlds='elsewhere'),
        'elsewhere: VecDrone2DEnv': lambda: vec_env.VecDrone2DEnv(p, 2, backend=oracle, worlds='elsewhere'),
        # three worlds for one setting
        'count: vo_feasibility_batch': lambda: metrics.vo_feasibility_batch([index], backend=vo_model, worlds=[None] * 3),
        'count: traversibility_batch': lambda: metrics.traversibility_batch([index], backend=model, worlds=[None] * 3),
        'count: survival_fit_batch': lambda: metrics.survival_fit_batch([index], backend=model, worlds=[None] * 3),
        'count: survivability_table': lambda: sweeps.survivability_table(*ONE, backend=oracle, worlds=[None] * 3),
        'count: vo_table': lambda: metrics.vo_table(*ONE, backend=vo_model, worlds=[None] * 3),
        'count: density_table': lambda: metrics.density_table(*ONE, worlds=[None] * 3),
        'count: traversibility_table': lambda: metrics.traversibility_table(*ONE, backend=model, worlds=[None] * 3),
        'count: survival_fit_table': lambda: metrics.survival_fit_table(*ONE, backend=model, worlds=[None] * 3),
        # a library that is not there
        'not found: load_library': lambda: _lib.load_library(_lib.LIB_PATH + '.absent'),
        'not found: load_worlds_library': lambda: _lib.load_worlds_library(_lib.WORLDS_LIB_PATH + '.absent'),
        'not found: load_metrics_library': lambda: _lib.load_metrics_library(_lib.METRICS_LIB_PATH + '.absent'),
    }
    out = {name: _refusal(call) for name, call in calls.items()}
    # a library of another version: the built one, against an expectation of 99
    for name, const, load in (('load_library', 'D2D_ABI_VERSION', _lib.load_library),
                              ('load_worlds_library', 'D2D_WORLDS_VERSION', _lib.load_worlds_library),
                              ('load_metrics_library', 'D2D_METRICS_VERSION', _lib.load_metrics_library)):
        with _patched(A, const, 99):
            out['mismatch: ' + name] = _refusal(load)
    # a return code that is not 0, through the one entry point that needs no GPU
    cfg = A.Cfg()
    out['rc != 0: launch_shape'] = _refusal(lambda: _lib.launch_shape(cfg))
    # the key sets of the timings
    for name, batch in (('traversibility_batch', metrics.traversibility_batch), ('survival_fit_batch', metrics.survival_fit_batch)):
        tm = {}
        batch([index], backend=model, timings=tm)
        out['timings: ' + name] = sorted(tm)
        out['timings batch: ' + name] = sorted(tm['batches'][0])
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_texts_are_the_recorded_ones(pkg, oracle, golden):
    got = record(pkg, oracle)
    assert sorted(got) == sorted(golden)
    for name, row in got.items():
        assert row == golden[name], name


def test_recording_holds_what_it_is_for(golden):
    kinds = {name: row[0] for name, row in golden.items() if not name.startswith('timings')}
    assert {k for n, k in kinds.items() if n.startswith('no kernels')} == {'NotImplementedError'}
    assert {k for n, k in kinds.items() if n.startswith(('elsewhere', 'count'))} == {'ValueError'}
    assert {k for n, k in kinds.items() if n.startswith(('not found', 'mismatch', 'rc != 0'))} == {'D2DError'}
    assert all('<root>' in golden['not found: ' + n][1] and 'build.sh' in golden['not found: ' + n][1]
               for n in ('load_library', 'load_worlds_library', 'load_metrics_library'))
    assert [golden['mismatch: ' + n][1].split(':')[0] for n in ('load_library', 'load_worlds_library', 'load_metrics_library')] == \
        ['libd2d_hip.so ABI 8 != expected 99', 'libd2d_worlds.so version 1 != expected 99', 'libd2d_metrics.so version 2 != expected 99']
    assert golden['rc != 0: launch_shape'][1].startswith('d2d error -')
    assert len({golden[f'elsewhere: {n}'][1] for n in ('vo_feasibility_batch', 'traversibility_batch', 'survival_fit_batch',
                                                       'survivability_batch')}) == 1
