"""swept_obs, seen_obs and scan_obs switched on together, on the device (libd2d_hip.so, libd2d_seen.so and libd2d_scan.so on one
stream, with the RVO, Jerk_Primitive and gaze libraries where the cell has them): the cases of tests/obs_channels_cases.py, which
tests/test_obs_channels_cpu.py runs on the model backends.  Streams with each channel alone -- what the per-channel suites tie to the
models and the reference -- against streams with all three, and every step path with every channel it admits against twins with one
channel, against the env without any and, where no channel had run on the device before, against the models.  Every comparison is
exact equality: integers, and the bit patterns of floats."""
import pytest

import action_stream_cases as AC
import obs_channels_cases as OC
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu


@pytest.fixture
def make(hip):
    def env_of(p, n, **kw):
        from drone2d_amd import vec_env
        kw.setdefault('gaze', 'external')
        kw.setdefault('device_plugins', True)
        kw.setdefault('planner', p.planner)
        kw.setdefault('worlds', 'device')
        return vec_env.VecDrone2DEnv(p, n, backend=hip, **kw)
    return env_of


# ---------------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_streams_with_each_channel_alone_against_all_three(pkg, make, cell):
    """8 slots, 24 episodes, a turn every 4 steps, six streams.  With all three channels Primitive-CVM leaves the persistent kernel for
    the per-stage step, and the seen and scan launches follow a _plugins_step of a stream for the first time"""
    slots, M = 8, 24
    p = AC.params_of(pkg, cell)
    cov = OC.stream_matrix(make, p, slots, M)
    OC.check_stream_coverage(cov, slots, M, swept_marks=p.planner == 'Primitive')


def test_stream_episodes_with_all_three_against_none(pkg, make):
    """the device's own policy, refilled through _refill_rest: _swept_zero, reset_plugins, _seen_zero (with its launch) and _scan_zero"""
    p = AC.params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    assert OC.stream_episodes_pair(make, p, 8, 24) == 24 - 8


# ---------------------------------------------------------------------------------------------------------------- step paths
STEP_PATHS = {     # cell -> (Params keywords, env keywords, the channels step() admits)
    'Primitive-CVM': ({}, {}, ('seen', 'scan')),      # (step() runs no plan stage: the swept launches are never queued)
    'Primitive-RVO': ({}, {}, ('seen', 'scan')),
    'Jerk-CVM': ({}, {}, OC.CHANNELS),                # (the swept crop of Jerk_Primitive is zero by definition)
    'NoMove': (dict(planner='NoMove'), dict(device_plugins=False, gaze=None), ('seen', 'scan')),
}


@pytest.mark.parametrize('cell', list(STEP_PATHS))
def test_step_with_every_channel_it_admits(pkg, make, cell):
    pkw, ekw, channels = STEP_PATHS[cell]
    p = AC.params_of(pkg, 'Primitive-CVM' if cell == 'NoMove' else cell, **pkw)
    full, _, _ = OC.path_case(make, p, lambda env, act: env.step(act), channels, env_kw=ekw)
    assert bool(full.seen['obs'].any()) and bool(full.scan['obs'].any())


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO'])
def test_the_per_stage_step_with_all_three(pkg, make, cell):
    full, _, _ = OC.path_case(make, AC.params_of(pkg, cell), OC.plugins_step, OC.CHANNELS)
    assert bool(full.state.flags[:, A.F_DONE].all()) and all(bool(getattr(full, c)['obs'].any()) for c in OC.CHANNELS)


def test_perceive_then_act(pkg, make):
    """the rays behind perceive(), age_map behind act(): against scan_model and seen_model on two envs per step, and against twins"""
    full, kinds = OC.perceive_act_case(make, AC.params_of(pkg, 'Primitive-CVM'))
    assert kinds[2] > 0 and kinds[3] > 0


def test_closed_loop_of_one_step_with_the_scan(pkg, make):
    """the persistent kernel with the snapshot in front and the scan launch behind: against scan_model and a _plugins_step twin"""
    full, kinds = OC.closed_loop_case(make, AC.params_of(pkg, 'Primitive-CVM'))
    assert bool(full.state.flags[:, A.F_DONE].all()) and kinds[2] > 0 and kinds[3] > 0


def test_policy_step_and_run_episodes_under_oxford(pkg, make):
    compared, frozen = OC.oxford_case(make, AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'))
    assert compared >= 4 * OC.B_PATH and frozen >= 1


def test_reset_of_half_the_envs_in_mid_episode(pkg, make):
    OC.reset_case(make, AC.params_of(pkg, 'Primitive-CVM'))
