"""The Jerk_Primitive step of VecDrone2DEnv and Drone2DEnv2 without a GPU: the CPU oracle for the stages of include/d2d.h, the host
build of csrc/jerk/d2d_jerk.h for the plan (tests/jerk_backend.py), every recorded world step for step.  test_gpu_jerk_env.py runs the
same replays on the device."""
import numpy as np
import pytest

import host_build
import jerk_env_cases as EC
import jerk_model as M

pytestmark = host_build.needs_fma('numpy takes non-FMA norm variants on this CPU')


@pytest.fixture(scope='module')
def backend():
    from jerk_backend import OracleJerkBackend
    return OracleJerkBackend()


# the oracle has no RVO stage and draws no measurement noise: test_gpu_jerk_env.py replays those two worlds, and the facade test
# below replays var_cam2 with the host's draws
ORACLE_WORLDS = [i for i, n in enumerate(EC.world_names()) if n not in ('rvo', 'var_cam2')]


@pytest.mark.parametrize('i', ORACLE_WORLDS, ids=[EC.world_names()[i] for i in ORACLE_WORLDS])
def test_vec_env_replays_every_recorded_step(pkg, backend, i):
    env = EC.replay_vec(pkg, backend, i, B=2)
    assert env.jerk.unknown_patterns() == 0


def test_reset_mid_episode_then_replays(pkg, backend):
    i = EC.world_names().index('default20')
    EC.replay_vec(pkg, backend, i, B=2, reset_at=30)


def test_perceive_plus_act_is_step(pkg, backend):
    from drone2d_amd import vec_env
    i = EC.world_names().index('obstacle_map')
    w = EC.world(i)
    p = EC.params_of(pkg, w)
    env = vec_env.VecDrone2DEnv(p, 1, backend=backend, planner='Jerk_Primitive', device_plugins=True, jerk_tie=EC.tie_table())
    for t in range(12):
        env.perceive()
        env.act(w['actions'][t])
        EC.check_step(w, t, env.state, env.jerk)


def test_rollout_is_a_loop_of_steps(pkg, backend):
    from drone2d_amd import vec_env
    i = EC.world_names().index('default40')
    w = EC.world(i)
    p = EC.params_of(pkg, w)
    env = vec_env.VecDrone2DEnv(p, 1, backend=backend, planner='Jerk_Primitive', device_plugins=True, jerk_tie=EC.tie_table())
    env.rollout(w['actions'][:10, None])
    EC.check_step(w, 9, env.state, env.jerk)


def test_rotating_and_nocontrol_keep_their_constant_action(pkg, backend):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='Jerk_Primitive', agent_number=3, map_id=1)
    for gaze, a in (('Rotating', 1.0), ('NoControl', 0.0)):
        env = vec_env.VecDrone2DEnv(p, 2, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze=gaze)
        assert env.state.action.tolist() == [a, a]
        env.run_step()
        assert env.state.plan_ok.tolist() == [1, 1] and (env.jerk_choice >= 0).all() and (env.jerk_stat >> 8 >= 1).all()


@pytest.mark.parametrize('name', ['two_targets', 'var_cam2', 'tie'])
def test_facade_replays_the_episode_after_enable_device_jerk(pkg, backend, device_jerk, name):
    from drone2d_amd import env as envmod, planners
    i = EC.world_names().index(name)
    w = EC.world(i)
    p = EC.params_of(pkg, w)
    e = envmod.Drone2DEnv2(p, backend=backend)
    assert isinstance(e.planner, planners.Jerk_Primitive) and e._mode == 'jerk'
    e._vec.jerk.tables['tie_perm'].copy_(__import__('torch').from_numpy(EC.tie_table()[0]))
    for t in range(len(w['t_done'])):
        _, _, done, info = e.step(w['actions'][t])
        assert len(e.planner.trajectory) == 0
        assert M.bits_equal([e.drone.x, e.drone.y, e.drone.yaw], w['t_drone'][t]), t
        assert M.bits_equal(np.concatenate([e.drone.velocity, e.drone.acceleration]), w['t_vel'][t]), t
        assert e.state_machine == w['t_sm'][t] and e.fail_count == w['t_fail'][t] and done == bool(w['t_done'][t]), t
        assert [info['collision_flag'], info['dead_lock_flag'], info['freezing_flag']] == w['t_flags'][t].tolist(), t
        assert M.bits_equal(e.planner.target[:2], w['t_p_target'][min(t + 1, len(w['t_done']) - 1)]) or w['t_sm'][t] in (0, 1), t


@pytest.fixture
def device_jerk():
    """registers the device Jerk_Primitive and always takes it out again"""
    from drone2d_amd import planners
    planners.enable_device_jerk()
    try:
        yield
    finally:
        planners.enable_device_jerk(False)
