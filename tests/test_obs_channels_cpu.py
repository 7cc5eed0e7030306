"""swept_obs, seen_obs and scan_obs switched on together, without a GPU (the combined model backends of
tests/obs_channels_backend.py): streams with each channel alone against streams with all three, every step path with every channel
it admits, the order of the launches of a step, reset and refill, and the restore list at its widest.  The cases are those of
tests/obs_channels_cases.py, which tests/test_gpu_obs_channels.py runs on the HIP libraries.  Every comparison is exact equality:
integers, and the bit patterns of floats."""
import pytest
import torch

import action_stream_cases as AC
import obs_channels_backend as CB
import obs_channels_cases as OC
from drone2d_amd import _abi as A


def make(params, n, **kw):
    """device worlds on the combined turn backend; an env without plugins (NoMove) on the combined oracle backend"""
    if kw.get('device_plugins', True) is False:
        return CB.env_of(params, n, **kw)
    return CB.stream_env_of(params, n, **kw)


# ---------------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_streams_with_each_channel_alone_against_all_three(pkg, cell):
    """3 slots, 9 episodes, a turn every 4 steps, six streams.  (Jerk-CVM: 12 episodes, the count at which tests/action_stream_cases.py
    chose the cell's map ids to hold a collision: the first nine of them all end by freezing)"""
    slots, M = 3, 12 if cell == 'Jerk-CVM' else 9
    p = AC.params_of(pkg, cell)
    cov = OC.stream_matrix(make, p, slots, M)
    OC.check_stream_coverage(cov, slots, M, swept_marks=p.planner == 'Primitive')


def test_stream_episodes_with_all_three_against_none(pkg):
    p = AC.params_of(pkg, 'Primitive-CVM', gaze_method='Rotating')
    assert OC.stream_episodes_pair(make, p, 2, 5) >= 3


# ---------------------------------------------------------------------------------------------------------------- step paths
STEP_PATHS = {     # cell -> (Params keywords, env keywords, the channels step() admits)
    'Primitive-CVM': ({}, {}, ('seen', 'scan')),      # (step() runs no plan stage: the swept launches are never queued)
    'Primitive-RVO': ({}, {}, ('seen', 'scan')),
    'Jerk-CVM': ({}, {}, OC.CHANNELS),                # (the swept crop of Jerk_Primitive is zero by definition)
    'NoMove': (dict(planner='NoMove'), dict(device_plugins=False, gaze=None), ('seen', 'scan')),
}


@pytest.mark.parametrize('cell', list(STEP_PATHS))
def test_step_with_every_channel_it_admits(pkg, cell):
    pkw, ekw, channels = STEP_PATHS[cell]
    p = AC.params_of(pkg, 'Primitive-CVM' if cell == 'NoMove' else cell, **pkw)
    full, _, _ = OC.path_case(make, p, lambda env, act: env.step(act), channels, env_kw=ekw)
    assert bool(full.seen['obs'].any()) and bool(full.scan['obs'].any())


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO'])
def test_the_per_stage_step_with_all_three(pkg, cell):
    full, _, _ = OC.path_case(make, AC.params_of(pkg, cell), OC.plugins_step, OC.CHANNELS)
    assert bool(full.state.flags[:, A.F_DONE].all()) and all(bool(getattr(full, c)['obs'].any()) for c in OC.CHANNELS)


def test_perceive_then_act(pkg):
    full, kinds = OC.perceive_act_case(make, AC.params_of(pkg, 'Primitive-CVM'))
    assert kinds[2] > 0 and kinds[3] > 0


def test_closed_loop_of_one_step_with_the_scan(pkg):
    full, kinds = OC.closed_loop_case(make, AC.params_of(pkg, 'Primitive-CVM'))
    assert bool(full.state.flags[:, A.F_DONE].all()) and kinds[2] > 0 and kinds[3] > 0


def test_policy_step_and_run_episodes_under_oxford(pkg):
    compared, frozen = OC.oxford_case(make, AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'))
    assert compared >= 4 * OC.B_PATH and frozen >= 1


def test_reset_of_half_the_envs_in_mid_episode(pkg):
    OC.reset_case(make, AC.params_of(pkg, 'Primitive-CVM'))


# ---------------------------------------------------------------------------------------------------------------- the launch order
STEP = ['snapshot', 'perceive', 'swept_mark', 'plan', 'act', 'swept_crop', 'seen_update', 'scan_update']
NOT_A_STAGE = ('gaze_stage_live', 'gaze_act', 'rvo_velocity', 'rvo_agents_step', 'rvo_velocity_live', 'rvo_agents_step_live')


def _logged(env, fn):
    """the launches fn() queues on `env`, in order and in the words of STEP: the pose snapshot, the perceive, plan and act launches
    and the channels' own (the gaze and RVO launches in front of the perceive launch are left out)"""
    orig = env._scan_snapshot
    env.backend.log = log = []
    env._scan_snapshot = lambda: (log.append('snapshot'), orig())[1]
    try:
        fn()
    finally:
        env.backend.log = None
        env._scan_snapshot = orig
    return [n for n in log if n not in NOT_A_STAGE]


def test_with_all_three_every_path_queues_each_launch_once_per_step_and_in_order(pkg):
    act = torch.zeros(2, dtype=torch.float64)
    p = AC.params_of(pkg, 'Primitive-CVM')
    env = make(p, 2, **OC.keywords(OC.CHANNELS))
    assert _logged(env, env._plugins_step) == STEP
    assert _logged(env, lambda: env._episode_steps(3)) == STEP * 3
    stream = make(p, 2, **OC.keywords(OC.CHANNELS)).action_stream(4)
    assert _logged(stream.env, lambda: stream.step(act)) == STEP
    rvo = make(AC.params_of(pkg, 'Primitive-RVO'), 2, **OC.keywords(OC.CHANNELS))
    assert _logged(rvo, rvo._plugins_step) == STEP and _logged(rvo, lambda: rvo._episode_steps(2)) == STEP * 2
    ox = make(AC.params_of(pkg, 'Primitive-CVM', gaze_method='Oxford'), 2, gaze='Oxford', **OC.keywords(OC.CHANNELS))
    assert _logged(ox, ox.policy_step) == STEP and _logged(ox, lambda: ox.run_episodes(max_steps=3)) == STEP * 3
    # the paths that admit seen and scan alone: no swept launch, the other two behind the step
    both = make(p, 2, seen_obs=True, scan_obs=True)
    tail = ['seen_update', 'scan_update']
    assert _logged(both, lambda: both._episode_steps(2)) == (['snapshot', 'closed_loop'] + tail) * 2
    assert _logged(both, lambda: both.step(act)) == ['snapshot', 'step'] + tail
    assert _logged(both, both.perceive) == ['snapshot', 'perceive', 'scan_update'] and _logged(both, lambda: both.act(act)) == ['act', 'seen_update']
    jerk = make(AC.params_of(pkg, 'Jerk-CVM'), 2, **OC.keywords(OC.CHANNELS))
    assert _logged(jerk, lambda: jerk._episode_steps(2)) == (['snapshot', 'perceive', 'plan', 'act'] + tail) * 2
    assert _logged(jerk, lambda: jerk.step(act)) == ['snapshot', 'perceive', 'plan', 'act'] + tail


# ---------------------------------------------------------------------------------------------------------------- the restore list
def test_the_restore_list_at_its_widest(pkg):
    """Primitive under RVO, a static map whose cell agents make N > agent_number, var_cam != 0 (rng_draws) and all three channels:
    the list names every buffer _refill_rest clears, once each, fits D2D_RESTORE_MAX_ITEMS and packs; and the turn's sequence over
    it (restore, the masked resets, the seen launch) leaves what _refill_rest leaves, in every tensor and every channel"""
    from drone2d_amd import action_stream
    from test_action_stream_cpu import STATIC, expected_items
    p = AC.params_of(pkg, 'Primitive-RVO', **dict(STATIC, var_cam=2))
    envs = [make(p, 4, **OC.keywords(OC.CHANNELS)) for _ in range(2)]
    for env in envs:                               # the model backends draw no noise on the device: the stream's field is named all the same
        env.state.t['rng_draws'] = torch.zeros((4, env.cfg.N, 2), dtype=torch.float64)
        env.set_noise(torch.zeros((4, env.cfg.N, 2), dtype=torch.float64))
    env = envs[1]
    N, k = env.cfg.N, min(p.agent_number, env.cfg.N)
    assert N > k
    prev = torch.full((4,), 7, dtype=torch.int32)
    items = action_stream.restore_items(env, prev)
    names = [i.name for i in items]
    sc = env.plugins.scalars
    want = [n for n, *_ in expected_items('Primitive-RVO', N, k, env.cfg.L, sc['traj_cap'], sc['node_cap'], sc['hash_cap'], True)]
    channels = ['swept.map', 'swept.obs', 'swept.count', 'seen.seen', 'seen.last_call'] + ['scan.' + n for n in A.SCAN_OUTPUTS]
    assert names == want[:-1] + channels + want[-1:] and len(set(names)) == len(names) == 30
    assert len({(i.dst.data_ptr(), i.dst_off) for i in items}) == len(items)           # no range twice
    by_name = {i.name: i for i in items}
    for name in channels:
        c, n = name.split('.')
        assert by_name[name].dst is getattr(env, c)[n] and by_name[name].kind == A.RESTORE_ZERO
        assert by_name[name].bytes == by_name[name].dst[0].numel() * by_name[name].dst.element_size(), name
    assert len(items) <= A.RESTORE_MAX_ITEMS
    packed, n = action_stream.pack_items(items, 'cpu')
    assert n == len(items)
    # the same refill through either route
    act = torch.linspace(-1, 1, 4, dtype=torch.float64)
    for e_ in envs:
        for _ in range(3):
            OC.plugins_step(e_, act)
    assert all(bool(getattr(envs[0], c)['obs'].any()) for c in OC.CHANNELS)
    refill = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    envs[0]._refill_rest(refill)
    packed, n = action_stream.pack_items(action_stream.restore_items(env, prev), 'cpu')      # (the velocity buffers have swapped)
    env.backend.stream_restore(packed, n, refill)
    env.reset_plugins(refill)
    env._seen_update()
    assert prev.tolist() == [0, 7, 0, 7]
    assert OC.differing(OC.state_of(envs[0]), OC.state_of(env)) == []
    for c in OC.CHANNELS:
        a, b = OC.records(envs[0], c), OC.records(env, c)
        a.pop('live', None), b.pop('live', None)   # (the mark rewrites the live bytes of every env in front of every plan)
        assert OC.differing(a, b) == [], c
    for e in (0, 2):                               # (no world was rebuilt: the seen launch has marked the pose the slot stands in)
        OC.check_fresh(env, e, ('swept', 'scan'))
        assert int(env.seen['last_call'][e]) == 4 and set(env.seen_calls[e].unique().tolist()) == {0, 4}
    assert int(env.scan['last_step'][1]) == 3 and bool(env.swept['map'][1].any())
