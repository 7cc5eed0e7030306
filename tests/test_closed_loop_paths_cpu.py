"""The case table of tests/test_gpu_closed_loop_paths.py without a GPU: every row builds the d2d_cfg / d2d_plan of its batch and
takes the d2d_closed_loop path it declares (d2d_launch_shape needs no GPU), and the table covers every (path, gaze),
(path, on_done) and (gaze, on_done) pair, with the noise, tiling, size and traj_box rows the GPU file relies on."""
import itertools

import pytest

import closed_loop_cases as CL


@pytest.mark.parametrize('case', CL.CASES, ids=CL.case_id)
def test_row_takes_its_declared_path(pkg, case):
    cfg, plan = CL.cfg_and_plan(pkg, case)
    assert CL.closed_loop_path(cfg, plan) == case['path']
    assert cfg.B == case['B'] and (cfg.sigma != 0) == case['noise']
    if case['layout'] == 'tiled':                       # partial edge tiles
        assert cfg.grid_tile == 16 and cfg.W % 16 and cfg.H % 16
    assert (plan.traj_box is None) == case['null_box']


def test_path_helper_follows_the_dispatch(pkg):
    """closed_loop_path() on variations of one row: the persistent path needs launch_args and a device plugin, NoMove is always
    per stage, var_cam != 0 and tiled grids leave the specialised kernels, and the agent count picks the specialisation."""
    from drone2d_amd import _abi as A
    base = CL.CASES[0]
    assert base['path'] == 'k_closed<1>'

    def path(**change):
        c = dict(base, **{k: v for k, v in change.items() if k in base})
        c['kw'] = dict(base['kw'], **{k: v for k, v in change.items() if k not in base})
        return CL.closed_loop_path(*CL.cfg_and_plan(pkg, c))
    assert path(agent_number=16) == 'k_closed<1>' and path(agent_number=17) == 'k_closed<2>'
    assert path(agent_number=40) == 'k_closed<2>' and path(agent_number=41) == 'k_closed<3>'
    assert path(var_cam=2, noise=True) == 'k_closed<0>' and path(layout='tiled') == 'k_closed<4>'
    assert path(max_flight_time=79) == 'k_closed<0>' and path(drone_view_range=100) == 'k_closed<0>'
    assert path(map_size=[512, 512], layout='tiled') == 'k_closed<4>'
    assert path(path='per_stage_primitive') == 'per_stage_primitive' and path(path='per_stage_nomove') == 'per_stage_nomove'
    cfg, plan = CL.cfg_and_plan(pkg, dict(base, gaze='constant', policy='Rotating'))
    plan.planner = A.PLAN_NONE                           # neither plugin on the device: nothing for the persistent kernel to run
    assert CL.closed_loop_path(cfg, plan) == 'per_stage_gaze'
    plan.gaze = A.GAZE_LOOKAHEAD
    assert CL.closed_loop_path(cfg, plan) == 'k_closed<1>'


def test_table_covers_every_pairing():
    rows = CL.CASES
    axes = dict(path=CL.PATHS, gaze=CL.GAZES, on_done=CL.ON_DONE)
    for a, b in (('path', 'gaze'), ('path', 'on_done'), ('gaze', 'on_done')):
        have = {(c[a], c[b]) for c in rows}
        want = set(itertools.product(axes[a], axes[b]))
        assert have == want, (a, b, sorted(want - have))
    assert len({CL.case_id(c) for c in rows}) == len(rows)
    # measurement noise on both generic kernels and both per-stage loops, once with more than 16 agents (st_tracker_quad)
    noisy = [c for c in rows if c['noise']]
    assert {c['path'] for c in noisy} >= {'k_closed<0>', 'k_closed<4>', 'per_stage_nomove', 'per_stage_primitive'}
    assert any(c['kw'].get('agent_number', 10) > 16 for c in noisy)
    for c in noisy:                                  # some call starts at a noise row other than 0 (d2d_cfg.noise_row0 != 0)
        starts = itertools.accumulate(CL.chunk_sizes(c)[:-1])
        assert any(n % CL.NOISE_ROWS for n in starts), CL.case_id(c)
    # sizes: B = 1 and the other batch sizes, one-step and odd multi-step calls, a closed_loop(0) call
    assert {c['B'] for c in rows} == {1, 3, 5, 6}
    sizes = {n for c in rows for n in CL.chunk_sizes(c)}
    assert 1 in sizes and any(n > 1 and n % 2 for n in sizes) and any(c['zero_call'] for c in rows)
    # heading gaze on a non-square map and at map_scale 20
    heading = [c for c in rows if c['gaze'] in ('LookAhead', 'LookGoal')]
    assert any(c['kw'].get('map_size', [500, 500])[0] != c['kw'].get('map_size', [500, 500])[1] for c in heading)
    assert any(c['kw'].get('map_scale') == 20 for c in heading)
    # NULL traj_box on both sides of the dispatch
    assert {c['path'] for c in rows if c['null_box']} == {'k_closed<0>', 'per_stage_primitive'}
    assert all(60 <= c['T'] <= 120 for c in rows)
