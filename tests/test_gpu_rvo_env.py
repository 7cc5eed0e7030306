"""VecDrone2DEnv / Drone2DEnv2 under motion_profile='RVO' on the HIP library: the recorded worlds of tests/golden/rvo_traces.npz step
by step (agents everywhere; grids, hit mask, flags and observation where stored), with host-built and device-built worlds; a seeded
soak against the CPU oracle + the Python model; rollout, reset, the facade with Experiment, and a CVM env next to an RVO env."""
import pytest

import rvo_cases as RC
import rvo_env_cases as EC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('i', range(len(RC.world_names())), ids=RC.world_names())
def test_step_reproduces_the_recorded_worlds(pkg, hip, i):
    EC.step_world(pkg, hip, i, copies=1 if i else 3)


@pytest.mark.parametrize('i', range(len(RC.world_names())), ids=RC.world_names())
def test_step_reproduces_the_recorded_worlds_built_on_the_device(pkg, hip, i):
    EC.step_world(pkg, hip, i, worlds='device')


def test_soak_against_the_oracle_and_the_model(pkg, hip):
    from rvo_backend import OracleRvoBackend
    EC.soak(pkg, hip, OracleRvoBackend())


def test_rollout_equals_steps(pkg, hip):
    EC.rollout_equals_steps(pkg, hip)


def test_rollout_draws_a_noise_row_per_step(pkg, hip):
    EC.rollout_draws_a_noise_row_per_step(pkg, hip)


def test_a_batch_of_no_envs_is_built_and_steps_nothing(pkg, hip):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=5, agent_radius=10, agent_max_speed=20, map_id=1, pillar_number=3)
    env = vec_env.VecDrone2DEnv(p, 0, backend=hip, worlds='device')
    assert tuple(env.state.pillars.shape) == (0, 3, 3) and tuple(env.state.agent_vel.shape) == (0, 2, 5)
    env._rvo_agents()                                      # launches nothing: d2d_rvo_velocity refuses B < 1


def test_reset_restores_velocities_of_the_masked_envs_only(pkg, hip):
    EC.reset_restores_masked_velocities(pkg, hip)


def test_facade_and_experiment_reproduce_the_recorded_episode(pkg, hip):
    EC.episode(pkg, hip, hip.device)


def test_a_cvm_env_next_to_an_rvo_env_equals_its_fixture(pkg, hip):
    EC.cvm_next_to_rvo(pkg, hip)
