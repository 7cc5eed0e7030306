"""Whole Primitive episodes under the RVO motion profile as a batch without a GPU: runner.SteppedExperimentBatch and
VecDrone2DEnv.run_episodes / policy_step over tests/stepped_backend.py (the CPU oracle's stages, the host RVO build, and the four
launches that leave finished envs alone restated as "call, then put back"), against the reference's own episodes
(tests/golden/primitive_rvo_episodes.npz) step for step and row for row.  The oracle has Oxford's gaze stage and the two constants;
test_gpu_primitive_rvo_episodes.py replays every world on the device."""
import pytest

import host_build
import primitive_rvo_cases as PC

fma = host_build.needs_fma('numpy takes non-FMA norm variants on this CPU')
ORACLE_WORLDS = [i for i, n in enumerate(PC.world_names()) if PC.world(i)['cfg']['gaze_method'] in PC.ORACLE_GAZE]


def test_the_fixture_holds_what_the_tests_need():
    names = PC.world_names()
    assert names == ['lookahead_success', 'lookahead_collision', 'lookahead_deadlock', 'oxford_freezing', 'owl_pillars',
                     'lookgoal_var_cam2', 'lookahead_drone20', 'rotating', 'nocontrol']
    w = {n: PC.world(i) for i, n in enumerate(names)}
    for n, d in w.items():
        c = d['cfg']
        assert (c['motion_profile'], c['agent_number'], c['agent_radius'], c['agent_max_speed']) == ('RVO', 10, 15, 20), n
        assert int(d['N']) == 10 and d['t_agent_pos'].shape == d['t_agent_vel'].shape == (len(d['t_done']), 10, 2), n
        assert d['t_done'][-1] and not d['t_done'][:-1].any() and float(d['ref_s_per_step']) > 0, n
    # the four endings, at the steps the reference gives
    assert w['lookahead_success']['row'][4] == 1 and len(w['lookahead_success']['t_done']) == 190
    assert w['lookahead_collision']['row'][6] == 1 and len(w['lookahead_collision']['t_done']) == 176
    assert w['lookahead_deadlock']['row'][8] == 1 and len(w['lookahead_deadlock']['t_done']) == 89
    assert w['oxford_freezing']['row'][7] == 1 and len(w['oxford_freezing']['t_done']) == 120
    assert w['owl_pillars']['cfg']['pillar_number'] == 3 and 't_owl_U' in w['owl_pillars'] and w['owl_pillars']['t_owl_U'].any()
    assert w['lookgoal_var_cam2']['cfg']['var_cam'] == 2 and w['lookahead_drone20']['cfg']['drone_max_speed'] == 20
    assert any((d['t_plan_ok'] == 0).any() for d in w.values()) and any(d['t_replanned'].any() for d in w.values())
    assert sorted(w[n]['cfg']['gaze_method'] for n in names if names.index(n) in ORACLE_WORLDS) == ['NoControl', 'Oxford', 'Rotating']
    assert w['rotating']['t_action'].all() and not w['nocontrol']['t_action'].any()


@fma
@pytest.mark.parametrize('i', ORACLE_WORLDS, ids=[PC.world_names()[i] for i in ORACLE_WORLDS])
def test_every_recorded_episode_the_oracle_can_play_step_for_step_and_its_row(pkg, i):
    PC.replay(pkg, 'oracle', i)


@fma
def test_envs_that_end_at_different_steps_stay_frozen_agents_and_velocities_included(pkg):
    """map ids 0, 1, 2 with a goal 180 px from the start end by collision, freezing and success"""
    p = pkg.Params(planner='Primitive', motion_profile='RVO', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, max_flight_time=12, map_id=0, target_list=[[50, 230]])
    ended = PC.staggered(pkg, 'oracle', p)
    assert min(ended.values()) >= 20 and max(ended.values()) == 119


def test_under_cvm_run_episodes_is_the_frozen_closed_loop(pkg):
    env = PC.cvm_equals_closed_loop(pkg, 'oracle', 4)
    assert not env.rvo and env.step_gaze == 'Oxford'


@fma
def test_a_masked_reset_between_chunks_starts_a_fresh_policy_and_trajectory_for_that_env_alone(pkg):
    import torch
    from drone2d_amd import vec_env
    w = PC.world(PC.world_names().index('oxford_freezing'))
    p = PC.params_of(pkg, w)
    env = PC.env_of(pkg, 'oracle', p, 2, 'Oxford', worlds=[vec_env.build_worlds(p, 1)[0]] * 2)
    assert env.run_episodes(max_steps=12, check_every=4) == 12
    PC.check_step(w, 11, env, 0), PC.check_step(w, 11, env, 1)
    assert int(env.plugins.t['traj_hdr'][1, 1]) > 0 and bool(env.plugins.t['seen_step'][1].any())
    env.reset(torch.tensor([0, 1], dtype=torch.uint8))
    assert not env.plugins.t['traj_hdr'][1].any() and not env.plugins.t['seen_step'][1].any()
    for t in range(8):
        obs, reward, done, info = env.policy_step()
        PC.check_step(w, 12 + t, env, 0), PC.check_step(w, t, env, 1)
    assert done.shape == (2,) and 'flight_time' in info
    assert info['flight_time'].tolist() == pytest.approx([2.0, 0.8])


def test_the_refusals_keep_their_texts(pkg, oracle):
    from drone2d_amd import runner, vec_env
    from rvo_backend import OracleRvoBackend
    from stepped_backend import SteppedOracleBackend
    rvo = dict(planner='Primitive', motion_profile='RVO', agent_number=5, agent_radius=10, agent_max_speed=20, drone_max_speed=40, map_id=1)
    p = pkg.Params(gaze_method='Oxford', **rvo)
    # the persistent loop still refuses RVO, and now says where such episodes run
    env = PC.env_of(pkg, 'oracle', p, 2, 'Oxford')
    with pytest.raises(NotImplementedError, match='RVO') as e:
        env.closed_loop(3)
    assert all(s in str(e.value) for s in ('step()', 'Experiment', 'run_episodes()', 'SteppedExperimentBatch'))

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError('backend touched: ' + name)
    with pytest.raises(NotImplementedError, match='RVO') as e:
        runner.ExperimentBatch(p, 2, device='cpu', backend=Untouched())
    assert 'SteppedExperimentBatch' in str(e.value)
    # one batch runner per (planner, profile) cell
    with pytest.raises(NotImplementedError, match="runs planner 'Jerk_Primitive'"):
        runner.SteppedExperimentBatch(pkg.Params(planner='Primitive'), 2, device='cpu', backend=SteppedOracleBackend())
    with pytest.raises(NotImplementedError, match="runs planner 'Jerk_Primitive'"):
        runner.SteppedExperimentBatch(pkg.Params(gaze_method='Oxford', **dict(rvo, planner='NoMove')), 2, device='cpu',
                                      backend=SteppedOracleBackend())
    with pytest.raises(NotImplementedError, match='gaze_method'):
        runner.SteppedExperimentBatch(pkg.Params(gaze_method='MPC', **rvo), 2, device='cpu', backend=SteppedOracleBackend())
    # a backend without the launches that leave finished envs alone is refused by name, before any world is built
    with pytest.raises(NotImplementedError, match='d2d_stepped.h'):
        runner.SteppedExperimentBatch(p, 2, device='cpu', backend=OracleRvoBackend())
    plain = vec_env.VecDrone2DEnv(p, 2, backend=OracleRvoBackend(), planner='Primitive', device_plugins=True, gaze='Oxford')
    with pytest.raises(NotImplementedError, match='d2d_stepped.h') as e:
        plain.run_episodes(1)
    assert 'oracle+rvo_host' in str(e.value)

    class NoRvoLive(SteppedOracleBackend):
        name = 'no_rvo_live'
        supports_rvo_live = False
    with pytest.raises(NotImplementedError, match='d2d_rvo_live.h') as e:
        PC.env_of(pkg, NoRvoLive(), p, 2, 'Oxford').policy_step()
    assert 'no_rvo_live' in str(e.value)
    # the caller's own gaze: no policy to step
    q = pkg.Params(gaze_method='Oxford', **dict(rvo, motion_profile='CVM'))
    ext = vec_env.VecDrone2DEnv(q, 2, backend=oracle, planner='Primitive', device_plugins=True, gaze='external')
    with pytest.raises(RuntimeError, match=r'policy_step\(\)'):
        ext.policy_step()
    with pytest.raises(RuntimeError, match=r'run_episodes\(\)'):
        ext.run_episodes()


@pytest.mark.parametrize('gaze,value', [('Rotating', 1.0), ('NoControl', 0.0)])
def test_the_constant_policies_launch_no_gaze_stage(pkg, gaze, value):
    from drone2d_amd import _abi as A
    p = pkg.Params(planner='Primitive', motion_profile='RVO', gaze_method=gaze, agent_number=5, agent_radius=10, agent_max_speed=20,
                   drone_max_speed=40, map_id=1)
    env = PC.env_of(pkg, 'oracle', p, 2, gaze)
    env.backend.gaze_stage_live = None                 # calling it would raise
    assert env._plan.gaze == A.GAZE_NONE and env.step_gaze == gaze
    env.policy_step()
    assert env.state.action.tolist() == [value, value] and env.state.counters[:, A.C_STEPS].tolist() == [1, 1]
