"""Whole Jerk_Primitive episodes as a batch without a GPU: runner.SteppedExperimentBatch and VecDrone2DEnv.run_episodes over the CPU
oracle for the stages of include/d2d.h, the host build of the planner and the host build of the gaze decision
(tests/gaze_backend.py), against the reference's own episodes (tests/golden/jerk_gaze_episodes.npz) step for step and row for row.
test_gpu_jerk_episodes.py runs the same replays on the device."""
import pytest

import host_build
import jerk_gaze_cases as EC

pytestmark = host_build.needs_fma('numpy takes non-FMA norm variants on this CPU')


@pytest.fixture(scope='module')
def backend():
    from gaze_backend import OracleGazeBackend
    return OracleGazeBackend()


# the oracle has no RVO stage and draws no measurement noise (as in test_jerk_env_cpu.py): test_gpu_jerk_episodes.py replays those two
ORACLE_WORLDS = [i for i, n in enumerate(EC.world_names()) if n not in ('owl_rvo', 'owl_var_cam2')]


def test_the_fixture_holds_what_the_tests_need():
    names = EC.world_names()
    for n in ('lookahead40', 'lookahead20', 'owl40', 'owl20', 'owl_var_cam2', 'owl_obstacle_map', 'owl_rvo', 'lookgoal', 'oxford',
              'nocontrol', 'rotating', 'freezing', 'deadlock'):
        assert n in names
    row = lambda n: EC.world(names.index(n))['row']                      # noqa: E731
    assert row('freezing')[7] == 1 and row('deadlock')[8] == 1 and row('owl40')[4] == 1
    for n in ('lookgoal', 'oxford'):
        assert not EC.world(names.index(n))['t_action'].any()
    assert EC.tie_table()[0].shape == (288, 72) and str(EC.traces()['numpy_version'])
    assert not any(EC.world(i)['t_unknown'].any() for i in range(len(names)))


@pytest.mark.parametrize('i', ORACLE_WORLDS, ids=[EC.world_names()[i] for i in ORACLE_WORLDS])
def test_every_recorded_episode_step_for_step_and_its_row(pkg, backend, i):
    EC.replay(pkg, backend, i)


def test_envs_that_end_at_different_steps_stay_frozen(pkg, backend):
    p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, max_flight_time=12, map_id=20)
    ended = EC.staggered(pkg, backend, p)
    assert min(ended.values()) >= 20


def test_the_refusals_are_unchanged(pkg, backend):
    from drone2d_amd import runner, vec_env
    from jerk_backend import OracleJerkBackend
    p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', agent_number=3, map_id=1)
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        vec_env.VecDrone2DEnv(p, 2, backend=OracleJerkBackend(), planner='Jerk_Primitive', device_plugins=True, gaze='Owl')
    assert str(e.value) == ("device plugins: planner 'Jerk_Primitive' / gaze 'Owl': the device Jerk_Primitive planner takes gaze "
                            "'external' (the caller's actions), 'Rotating' or 'NoControl'; drive any other policy from the host "
                            '(gaze.LookAhead, ...) and pass its actions to step()')
    with pytest.raises(NotImplementedError, match='SteppedExperimentBatch needs a backend'):
        runner.SteppedExperimentBatch(p, 2, device='cpu', backend=OracleJerkBackend())
    env = vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze='Owl')
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        env.closed_loop(3)
    assert str(e.value).startswith("closed_loop(): planner 'Jerk_Primitive' does not run inside the persistent closed loop (its stage "
                                   'lives in libd2d_jerk.so); step the env with step() / perceive() + act(), or run episodes through '
                                   'runner.Experiment')
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        class Untouched:
            def __getattr__(self, name):
                raise AssertionError('backend touched: ' + name)
        runner.ExperimentBatch(p, 2, device='cpu', backend=Untouched())
    assert str(e.value).startswith("ExperimentBatch: planner 'Jerk_Primitive' does not run inside the persistent closed loop (its stage "
                                   "lives in libd2d_jerk.so); step a VecDrone2DEnv(..., planner='Jerk_Primitive', device_plugins=True) "
                                   'with step(), or run the episodes through runner.Experiment, one at a time')
    with pytest.raises(NotImplementedError, match='MPC'):
        vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze='MPC')
    with pytest.raises(NotImplementedError, match="runs planner 'Jerk_Primitive'"):
        runner.SteppedExperimentBatch(pkg.Params(planner='Primitive'), 2, device='cpu', backend=backend)
    ext = vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True)
    with pytest.raises(RuntimeError, match='policy_step'):
        ext.policy_step()


def test_policy_step_is_a_gaze_launch_and_a_step_and_reset_starts_a_fresh_policy(pkg, backend):
    import torch
    from drone2d_amd import _abi as A, vec_env
    w = EC.world(EC.world_names().index('owl40'))
    p = EC.params_of(pkg, w)
    env = vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze='Owl', jerk_tie=EC.tie_table(),
                                worlds=[vec_env.build_worlds(p, 1)[0]] * 2)
    for t in range(12):
        obs, reward, done, info = env.policy_step()
        EC.check_step(w, t, env, 1)
    assert done.shape == (2,) and 'flight_time' in info
    env.reset(torch.tensor([0, 1], dtype=torch.uint8))
    assert not env.gaze_state.owl_state[1].any() and env.gaze_state.owl_state[0, :A.OWL_NDIR].any()
    env.reset()
    assert not env.gaze_state.owl_state.any()
    for t in range(10):
        env.policy_step()
        EC.check_step(w, t, env, 0)


@pytest.mark.parametrize('gaze,value', [('LookGoal', 0.0), ('Oxford', 0.0), ('Rotating', 1.0), ('NoControl', 0.0)])
def test_the_constant_policies_keep_a_resident_action(pkg, backend, gaze, value):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='Jerk_Primitive', gaze_method=gaze, agent_number=3, map_id=1)
    env = vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze=gaze)
    assert env.gaze_state is None and env.step_gaze == gaze
    env.policy_step()
    assert env.state.action.tolist() == [value, value]
