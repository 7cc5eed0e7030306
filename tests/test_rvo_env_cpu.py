"""VecDrone2DEnv / Drone2DEnv2 under motion_profile='RVO' without a GPU: the CPU oracle for the stages of include/d2d.h and the host
build of csrc/rvo/d2d_rvo.h for the two RVO entry points (rvo_backend.OracleRvoBackend), through the recorded worlds of
tests/golden/rvo_traces.npz.  The same cases run on the HIP library in test_gpu_rvo_env.py."""
import pytest

import host_build
import rvo_cases as RC
import rvo_env_cases as EC

pytestmark = host_build.needs_fma('numpy takes non-FMA norm / matmul variants on this CPU')


@pytest.fixture(scope='module')
def backend():
    from rvo_backend import OracleRvoBackend
    return OracleRvoBackend()


@pytest.mark.parametrize('i', range(len(RC.world_names())), ids=RC.world_names())
def test_step_reproduces_the_recorded_worlds(pkg, backend, i):
    EC.step_world(pkg, backend, i, copies=1 if i else 3)


def test_rollout_equals_steps(pkg, backend):
    EC.rollout_equals_steps(pkg, backend)


def test_rollout_draws_a_noise_row_per_step(pkg, backend):
    EC.rollout_draws_a_noise_row_per_step(pkg, backend)


def test_reset_restores_velocities_of_the_masked_envs_only(pkg, backend):
    EC.reset_restores_masked_velocities(pkg, backend)


def test_facade_and_experiment_reproduce_the_recorded_episode(pkg, backend):
    EC.episode(pkg, backend, 'cpu')


def test_a_cvm_env_next_to_an_rvo_env_equals_its_fixture(pkg, backend):
    EC.cvm_next_to_rvo(pkg, backend)
