"""Whole Jerk_Primitive episodes as a batch on the device (run with -m gpu): runner.SteppedExperimentBatch and
VecDrone2DEnv.run_episodes on the HIP backend -- libd2d_gaze.so, libd2d_rvo.so, libd2d_hip.so, libd2d_jerk.so, four or five launches a
step -- against the reference's own episodes (tests/golden/jerk_gaze_episodes.npz, every world, RVO and the drawn measurement noise
included) step for step and row for row, and against runner.Experiment with the host policies, which does not depend on the fixture."""
import copy

import numpy as np
import pytest

import jerk_gaze_cases as EC

pytestmark = pytest.mark.gpu
WORLDS = list(range(len(EC.world_names())))


@pytest.mark.parametrize('i', WORLDS, ids=EC.world_names())
def test_every_recorded_episode_step_for_step_and_its_row(pkg, hip, i):
    EC.replay(pkg, hip, i)


def test_envs_that_end_at_different_steps_stay_frozen(pkg, hip):
    p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, max_flight_time=12, map_id=20)
    EC.staggered(pkg, hip, p)


@pytest.fixture
def device_jerk():
    from drone2d_amd import planners
    planners.enable_device_jerk()
    try:
        yield
    finally:
        planners.enable_device_jerk(False)


@pytest.mark.parametrize('gaze', ['Owl', 'LookAhead'])
def test_sixty_four_envs_equal_sixty_four_experiments(pkg, hip, device_jerk, gaze):
    """map ids 0 .. 63 as one batch against 64 runs of runner.Experiment -- the device planner behind the facade, the policy evaluated
    on the host by gaze.Owl / gaze.LookAhead each step -- row for row.  A goal 180 px from the start keeps the 64 host-driven episodes
    (one env, one round trip per step) to some forty steps each"""
    from drone2d_amd import runner
    p = pkg.Params(planner='Jerk_Primitive', gaze_method=gaze, agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
                   max_flight_time=8, map_id=0, target_list=[[50, 230]])
    rows = runner.SteppedExperimentBatch(p, 64, backend=hip).run()
    assert len(rows) == 64 and len({r[12] for r in rows}) > 3 and sum(r[16] for r in rows) > 32
    for e in range(64):
        q = copy.copy(p)
        q.map_id = e
        one = runner.Experiment(q, backend=hip).run()
        a, b = rows[e], tuple(one)
        assert len(a) == len(b) == 22
        for k in range(22):
            x, y = a[k], b[k]
            same = (x != x and y != y) if isinstance(x, float) and x != x else x == y
            assert same or (k == 15 and abs(x - y) <= 1e-9), (e, k, a, b)     # column 15: see jerk_gaze_cases.check_row
