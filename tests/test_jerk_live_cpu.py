"""VecDrone2DEnv.run_episodes(live=...) with planner='Jerk_Primitive' without a GPU: the episode checks of tests/jerk_live_cases.py over
tests/jerk_live_backend.LiveJerkBackend (the CPU oracle, the host builds of the planner, the gaze decision and the RVO profile; the
masked launches made from the unmasked ones), under CVM and under RVO, and the sequence of launches each value of `live` makes on a
backend with and without the masked launches.  test_gpu_jerk_live_episodes.py runs the same checks on the device."""
import pytest

import host_build
import jerk_live_cases as LC
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend, Recording, UnmaskedBackend

pytestmark = host_build.needs_fma('numpy takes non-FMA norm variants on this CPU')
MAP_ID = {'CVM': LC.CVM_MAP_ID, 'RVO': LC.RVO_MAP_ID}


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_a_finished_env_is_its_own_single_env_episode_in_everything(pkg, profile):
    LC.a_finished_env_is_its_own_single_env_episode(pkg, LiveJerkBackend, LC.params(pkg, profile, MAP_ID[profile]))


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_everything_of_an_env_is_frozen_from_its_terminal_step_on(pkg, profile):
    LC.frozen_from_the_terminal_step_on(pkg, LiveJerkBackend, LC.params(pkg, profile, MAP_ID[profile]))


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_a_masked_reset_between_two_runs_starts_fresh_episodes_for_those_envs_alone(pkg, profile):
    LC.a_masked_reset_starts_fresh_episodes_for_those_envs_alone(pkg, LiveJerkBackend, LC.params(pkg, profile, MAP_ID[profile]))


def test_the_unmasked_loop_is_what_leaves_a_finished_env_s_plan_and_agents_behind(pkg):
    """the same check with live=False finds the buffers the masks are for: the loop of before has not quietly become masked"""
    with pytest.raises(AssertionError, match='s.agents') as e:
        LC.a_finished_env_is_its_own_single_env_episode(pkg, LiveJerkBackend, LC.params(pkg, 'RVO', LC.RVO_MAP_ID), live=False)
    assert 's.agent_vel' in str(e.value) and 's.wp' in str(e.value)


def test_the_rvo_map_id_is_the_first_of_its_search(pkg):
    """how RVO_MAP_ID was picked: the first of 0, 3, 6 ... whose three envs end at three different steps (one batch each; the
    search stops at the first hit, so this runs one batch when the constant is right)"""
    for map_id in range(0, 30, 3):
        env = LC.env_of(pkg, LiveJerkBackend, LC.params(pkg, 'RVO', map_id), 3)
        env.run_episodes()
        if len(set(LC.steps_played(env))) == 3:
            break
    assert map_id == LC.RVO_MAP_ID


PERCEIVE, ACT = A.ST_PERCEIVE | A.ST_SKIP_DONE, A.ST_ACT | A.ST_SKIP_DONE
PERCEIVE_RVO = (A.ST_PERCEIVE & ~A.ST_AGENTS) | A.ST_SKIP_DONE
BEFORE = {'CVM': ['gaze_act', ('run_stages', PERCEIVE), 'jerk_plan', ('run_stages', ACT)],
          'RVO': ['gaze_act', 'rvo_velocity', 'rvo_agents_step', ('run_stages', PERCEIVE_RVO), 'jerk_plan', ('run_stages', ACT)]}
MASKED = {'CVM': ['gaze_act', ('run_stages', PERCEIVE), 'jerk_plan_live', ('run_stages', ACT)],
          'RVO': ['gaze_act', 'rvo_velocity_live', 'rvo_agents_step_live', ('run_stages', PERCEIVE_RVO), 'jerk_plan_live', ('run_stages', ACT)]}


def recorded(pkg, inner, profile, **run):
    rec = Recording(inner())
    env = LC.env_of(pkg, rec, LC.params(pkg, profile, 1), 2)
    del rec.calls[:]
    assert env.run_episodes(max_steps=3, **run) == 3
    return rec.calls


@pytest.mark.parametrize('profile', ['CVM', 'RVO'])
def test_the_launches_of_a_step_for_every_value_of_live(pkg, profile):
    assert not hasattr(UnmaskedBackend, 'supports_jerk_live') and not hasattr(UnmaskedBackend, 'jerk_plan_live')
    # a backend without the masked launches: the loop of before under live=None, a refusal under live=True
    assert recorded(pkg, UnmaskedBackend, profile) == BEFORE[profile] * 3
    assert recorded(pkg, UnmaskedBackend, profile, live=False) == BEFORE[profile] * 3
    with pytest.raises(NotImplementedError, match='leaves finished envs alone') as e:
        recorded(pkg, UnmaskedBackend, profile, live=True)
    assert str(e.value) == ('oracle+jerk_host+gaze_host+rvo_host has no plan launch that leaves finished envs alone '
                            "(include/d2d_jerk_live.h): run_episodes(live=True) with planner 'Jerk_Primitive'" +
                            (' under RVO' if profile == 'RVO' else '') + ' runs on the HIP backend')
    # a backend with them: masked under None and True, the loop of before under False
    assert recorded(pkg, LiveJerkBackend, profile) == MASKED[profile] * 3
    assert recorded(pkg, LiveJerkBackend, profile, live=True) == MASKED[profile] * 3
    assert recorded(pkg, LiveJerkBackend, profile, live=False) == BEFORE[profile] * 3


def test_under_rvo_the_masked_loop_needs_both_libraries_masked_launches(pkg):
    class PlanOnly(LiveJerkBackend):
        name = 'plan_live_only'
        supports_rvo_live = False
    assert recorded(pkg, PlanOnly, 'RVO') == BEFORE['RVO'] * 3 and recorded(pkg, PlanOnly, 'CVM') == MASKED['CVM'] * 3
    with pytest.raises(NotImplementedError, match='include/d2d_rvo_live.h'):
        recorded(pkg, PlanOnly, 'RVO', live=True)
