"""seen_obs=True on the device (include/d2d_seen.h: d2d_seen_update of libd2d_seen.so): the reference's recorded maps through the
library step for step, handmade poses through the launch alone over poisoned buffers, a random soak against the numpy model of
tests/seen_model.py, the map against the one the Oxford stage keeps for itself, and action streams with the channel against the same
streams without it.  Every comparison is exact equality: integers, and the bit patterns of floats."""
import numpy as np
import pytest
import torch

import action_stream_cases as AC
import seen_cases as SC
import seen_model as SN
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu


def _env(hip, p, B, **kw):
    from drone2d_amd import vec_env
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', p.planner)
    return vec_env.VecDrone2DEnv(p, B, backend=hip, **kw)


def _step(env, action):
    env._set_action(action)
    env._plugins_step()


# ---------------------------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('i', range(SC.EPISODES))
def test_the_recorded_episodes_through_the_library(pkg, hip, i):
    assert hip.supports_seen_obs
    reseen, inside, never = SC.coverage()
    assert reseen >= 100 and inside >= 20 and never >= 1, (reseen, inside, never)
    ep = SC.episode(i)
    env = _env(hip, SC.params_of(pkg, ep), 1, seen_obs=True)
    assert SC.replay(env, ep, _step) == len(ep['action'])


# ---------------------------------------------------------------------------------------------------------------- 2. handmade
@pytest.mark.parametrize('k', range(5))
def test_handmade_poses_through_the_launch_alone(pkg, hip, k):
    """16 envs on the default map (corners, edges, a cell's origin, yaw 0 / 90 / 180 / 270 / 45, a finished env, a call beyond the
    table), maps of 30 x 20 and 20 x 30 cells, drone_view_depth 45 with 60 and 120 degree views: tests/seen_cases.handmade_sets"""
    p, view_range, poses = SC.handmade_sets(pkg)[k]
    env = _env(hip, p, len(poses), seen_obs=True, device_plugins=False, gaze=None)
    assert (env.cfg.W, env.cfg.H) == [(50, 50), (30, 20), (20, 30), (50, 50), (50, 50)][k]
    alone, marked, fresh = SC.run_handmade(env, view_range, poses, lambda: hip.seen_update(env.cfg, env._st, env._seen))
    assert alone == (2 if k == 0 else 0) and marked > 5 * len(poses) and 0 < fresh < marked


# ---------------------------------------------------------------------------------------------------------------- 3. random soak
def test_random_soak_against_the_model(pkg, hip):
    """64 device-built worlds x 100 steps, 30 agents at speed 40 and radius 10, random actions; the model keeps its own records from
    the poses and counters the device reports.  Coverage, not tolerance: envs that finished and stayed as they ended, and cells seen
    again after a gap, or the test has not looked where the launch can go wrong"""
    B, T = 64, 100
    p = pkg.Params(planner='Primitive', agent_number=30, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=2000, max_flight_time=8)
    env = _env(hip, p, B, seen_obs=True, worlds='device')
    cfg, tab = env.cfg, env.seen['tab'].cpu().numpy()
    gen = torch.Generator().manual_seed(13)
    seen, last = np.zeros((B, cfg.W, cfg.H), dtype=np.int32), np.zeros(B, dtype=np.int32)
    refreshed, obs = np.zeros(B, dtype=np.int32), np.zeros((B, cfg.L, cfg.L), dtype=np.float32)
    frozen = reseen = 0
    for t in range(T + 1):
        if t:
            _step(env, torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1)
        env.sync()
        drone, steps = env.state.drone.cpu().numpy(), env.state.counters[:, A.C_STEPS].cpu().numpy()
        for e in range(B):
            before = seen[e].copy()
            out = SN.update(seen[e], last[e], steps[e], drone[e], cfg, p.drone_view_range, tab)
            if out is None:
                frozen += 1
                continue
            last[e], refreshed[e], obs[e] = out
            reseen += int(((seen[e] == last[e]) & (before > 0) & (before < last[e] - 1)).sum())
        got = {k: env.seen[k].cpu().numpy() for k in ('seen', 'last_call', 'refreshed', 'obs')}
        assert np.array_equal(got['seen'], seen), (t, np.argwhere(got['seen'] != seen)[:5].tolist())
        assert np.array_equal(got['last_call'], last) and np.array_equal(got['refreshed'], refreshed), t
        assert np.array_equal(SC.bits(got['obs']), SC.bits(obs)), t
    assert bool(env.state.flags[:, A.F_DONE].all()) and frozen > B and reseen > 1000, (frozen, reseen)
    age = env.seen_age.cpu().numpy()
    assert all(np.array_equal(SC.bits(age[e]), SC.bits(SN.age_map(seen[e], int(last[e]), tab))) for e in range(B))


# ---------------------------------------------------------------------------------------------------------------- 4. the Oxford stage
def test_the_map_is_the_one_the_oxford_stage_keeps(pkg, hip):
    """env A decides with gaze='Oxford' (policy_step); env B takes A's actions as the caller's.  Before each of B's steps its records
    are A's seen_step behind A's gaze stage of that step, for the envs still playing"""
    B, T = 8, 60
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=40,
                   max_flight_time=8)
    a = _env(hip, p, B, gaze='Oxford')
    b = _env(hip, p, B, seen_obs=True)
    compared = 0
    for t in range(T):
        live = ~a.state.flags[:, A.F_DONE].bool()
        if not bool(live.any()):
            break
        assert torch.equal(b.state.drone[live], a.state.drone[live]), t      # the same worlds under the same actions so far
        a.policy_step()                    # the gaze stage marks seen_step from the pose of before the step; nothing later writes it
        assert torch.equal(b.seen_calls[live], a.plugins.t['seen_step'][live]), t
        compared += int(live.sum())
        _step(b, a.state.action.clone())
    assert compared > 4 * B and not bool(a.state.flags[:, A.F_DONE].logical_xor(b.state.flags[:, A.F_DONE]).any())


# ---------------------------------------------------------------------------------------------------------------- 5. the stream
@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_a_stream_with_the_channel_equals_the_stream_without(pkg, hip, cell):
    """8 slots, 24 episodes, a turn every 4 steps; a refilled slot shows the call-1 map at its step 0"""
    slots, M = 8, 24
    p = AC.params_of(pkg, cell)
    refills, frozen = SC.stream_pair(lambda q, n, seen: _env(hip, q, n, seen_obs=seen, worlds='device'), p, slots, M)
    assert refills == M - slots and frozen > 0


def test_the_library_refuses_what_it_cannot_hold(pkg, hip):
    import copy
    import ctypes as C
    env = _env(hip, AC.params_of(pkg, 'Primitive-CVM'), 1, seen_obs=True)
    hip.seen_update(env.cfg, env._st, env._seen)
    big = copy.copy(env.cfg)
    big.W, big.H = 32767, 32767 * 3
    assert hip.ofn['update'](C.byref(big), C.byref(env._st), C.byref(env._seen), None) == -4
    assert b'32-bit cell indices' in hip.ofn['last_error']()
    assert hip.ofn['update'](C.byref(env.cfg), C.byref(env._st), None, None) == -1
