"""Whole Primitive episodes under the RVO motion profile as a batch on the device (run with -m gpu): runner.SteppedExperimentBatch and
VecDrone2DEnv.run_episodes on the HIP backend -- the gaze and plan stages of libd2d_hip.so that leave finished envs alone
(include/d2d_stepped.h) around the RVO launches that do the same (include/d2d_rvo_live.h), five or six launches a step -- against the
reference's own episodes (tests/golden/primitive_rvo_episodes.npz, every world: the four endings, pillars under Owl, the drawn
measurement noise under LookGoal) step for step and row for row, and against runner.Experiment with the host policy, which does not
depend on the fixture.  Integers, flags, positions, velocities and the drone's fp64 state are held bit for bit; the row's mean
tracked time by jerk_gaze_cases.check_row's column rule."""
import copy

import pytest

import primitive_rvo_cases as PC

pytestmark = pytest.mark.gpu
WORLDS = list(range(len(PC.world_names())))


@pytest.mark.parametrize('i', WORLDS, ids=PC.world_names())
def test_every_recorded_episode_step_for_step_and_its_row(pkg, hip, i):
    PC.replay(pkg, hip, i)


def test_envs_that_end_at_different_steps_stay_frozen_agents_and_velocities_included(pkg, hip):
    """map ids 5, 6, 7 under Owl with a goal 180 px from the start: the reference ends them after 80, 67 and 61 steps"""
    p = pkg.Params(planner='Primitive', motion_profile='RVO', gaze_method='Owl', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, max_flight_time=8, map_id=5, target_list=[[50, 230]])
    ended = PC.staggered(pkg, hip, p)
    assert sorted(ended.values()) == [60, 66, 79]


def test_under_cvm_run_episodes_is_the_frozen_closed_loop_across_workgroups(pkg, hip):
    env = PC.cvm_equals_closed_loop(pkg, hip, 64, gaze='Owl')
    assert not env.rvo and env.num_envs == 64


def test_a_masked_reset_between_chunks_starts_a_fresh_policy_and_trajectory_for_that_env_alone(pkg, hip):
    import torch
    from drone2d_amd import vec_env
    w = PC.world(PC.world_names().index('owl_pillars'))
    p = PC.params_of(pkg, w)
    env = PC.env_of(pkg, hip, p, 2, 'Owl', worlds=[vec_env.build_worlds(p, 1)[0]] * 2)
    assert env.run_episodes(max_steps=12, check_every=4) == 12
    PC.check_step(w, 11, env, 0), PC.check_step(w, 11, env, 1)
    env.reset(torch.tensor([0, 1], dtype=torch.uint8))
    assert not env.plugins.t['traj_hdr'][1].any() and not env.plugins.t['owl_state'][1].any() and env.plugins.t['owl_state'][0].any()
    for t in range(8):
        env.policy_step()
        PC.check_step(w, 12 + t, env, 0), PC.check_step(w, t, env, 1)


def test_eight_envs_equal_eight_experiments(pkg, hip):
    """map ids 0 .. 7 as one batch against 8 runs of runner.Experiment -- one env, the RVO step behind the facade, the policy evaluated
    on the host by gaze.Owl each step -- row for row.  On these inputs the reference gives 80, 80, 67, 67, 67, 80, 67 and 61 steps:
    four successes, three freezes and one dead lock"""
    from drone2d_amd import runner
    p = pkg.Params(planner='Primitive', motion_profile='RVO', gaze_method='Owl', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, max_flight_time=8, map_id=0, target_list=[[50, 230]])
    xb = runner.SteppedExperimentBatch(p, 8, backend=hip)
    rows = xb.run()
    assert len(rows) == 8 and len({r[12] for r in rows}) >= 2 and sum(r[16] for r in rows) >= 1
    assert [round(r[12] / p.dt) for r in rows] == [80, 80, 67, 67, 67, 80, 67, 61] and xb.steps_run == 80
    for e in range(8):
        q = copy.copy(p)
        q.map_id = e
        one = runner.Experiment(q, backend=hip).run()
        a, b = rows[e], tuple(one)
        assert len(a) == len(b) == 22
        for k in range(22):
            x, y = a[k], b[k]
            same = (x != x and y != y) if isinstance(x, float) and x != x else x == y
            assert same or (k == 15 and abs(x - y) <= 1e-9), (e, k, a, b)     # column 15: see jerk_gaze_cases.check_row


def test_device_worlds_and_workers_build_the_same_batch(pkg, hip):
    from drone2d_amd import runner
    p = pkg.Params(planner='Primitive', motion_profile='RVO', gaze_method='LookAhead', agent_number=10, agent_radius=15,
                   agent_max_speed=20, drone_max_speed=40, max_flight_time=3, map_id=0, pillar_number=2)
    rows = [runner.SteppedExperimentBatch(p, 4, backend=hip, **kw).run() for kw in (dict(), dict(device_worlds=True))]
    assert rows[0] == rows[1] or all((a != a and b != b) or a == b for r, s in zip(*rows) for a, b in zip(r, s))
