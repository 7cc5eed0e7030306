"""Whole Jerk_Primitive episodes on the device with every launch leaving finished envs alone (run with -m gpu):
VecDrone2DEnv.run_episodes on the HIP backend with d2d_jerk_plan_live (include/d2d_jerk_live.h) and, under RVO, the launches of
include/d2d_rvo_live.h.  The checks are those of tests/jerk_live_cases.py, which test_jerk_live_cpu.py runs on the host builds.

Before the masked launches existed (run_episodes() without `live`: d2d_jerk_plan and the unmasked RVO launches for every env) these
tests were run once on that tree and failed, but for the masked reset under CVM: every env of the first test differed from its
one-env episode in s.wp and j.choice (and j.stat) under CVM, and in s.agents, s.wp, j.choice, j.stat (two of them also in s.agent_vel)
under RVO; the frozen test named the same buffers; the reset test under RVO found the agents and velocities of the two envs that were
not reset moved; the masked-against-unmasked tests had no `live` to pass."""
import pytest

import jerk_live_cases as LC

pytestmark = pytest.mark.gpu
MAP_ID = {'CVM': LC.CVM_MAP_ID, 'RVO': LC.RVO_MAP_ID}


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_a_finished_env_is_its_own_single_env_episode_in_everything(pkg, hip, profile):
    ended = LC.a_finished_env_is_its_own_single_env_episode(pkg, hip, LC.params(pkg, profile, MAP_ID[profile]))
    assert ended == {'CVM': [120, 101, 102], 'RVO': [102, 111, 101]}[profile]      # as on the host builds (test_jerk_live_cpu.py)


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_everything_of_an_env_is_frozen_from_its_terminal_step_on(pkg, hip, profile):
    LC.frozen_from_the_terminal_step_on(pkg, hip, LC.params(pkg, profile, MAP_ID[profile]))


@pytest.mark.parametrize('gaze', ['Owl', 'LookAhead'])
@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_masked_equals_unmasked_for_every_live_env_and_every_row(pkg, hip, profile, gaze):
    LC.masked_equals_unmasked(pkg, hip, profile, gaze)


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_a_masked_reset_between_two_runs_starts_fresh_episodes_for_those_envs_alone(pkg, hip, profile):
    LC.a_masked_reset_starts_fresh_episodes_for_those_envs_alone(pkg, hip, LC.params(pkg, profile, MAP_ID[profile]))


def test_live_true_and_the_default_are_the_masked_loop_on_this_backend(pkg, hip):
    assert hip.supports_jerk_live and hip.supports_rvo_live
    env = LC.env_of(pkg, hip, LC.params(pkg, 'RVO', 1), 2)
    assert env._jerk_live(None) is True and env._jerk_live(True) is True and env._jerk_live(False) is False
