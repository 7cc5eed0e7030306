"""scan_obs=True on the device (include/d2d_scan.h: d2d_scan_update of libd2d_scan.so): the reference's recorded rays through the
library step for step, handmade poses through the launch alone over poisoned buffers, BASELINE config 5's geometry in both grid
layouts, a random soak against the plain-Python model of tests/scan_model.py with the fused step's own hit union as a second
witness, and action streams with the channel against the same streams without it.  Every comparison is exact equality: integers,
and the bit patterns of floats."""
import numpy as np
import pytest
import torch

import action_stream_cases as AC
import scan_cases as SC
import scan_model as SN
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
    assert hip.supports_scan_obs
    SC.assert_coverage(SC.coverage())
    ep = SC.episode(i)
    env = _env(hip, SC.params_of(pkg, ep), 1, scan_obs=True, **SC.env_kw(ep))
    assert SC.replay(env, ep) == len(ep['action'])


# ---------------------------------------------------------------------------------------------------------------- 2. handmade
@pytest.mark.parametrize('k', range(len(SC.HANDMADE)))
def test_handmade_poses_through_the_launch_alone(pkg, hip, k):
    """16 envs (the corners, x == 0 and x == W_px, a cell's origin under yaw 0 / 45 / 90 / 135 / 270, inside one agent and inside two,
    a finished env and an env with counter 0) on maps of 50 x 50, 30 x 20 and -- tiled, with partial edge tiles -- 100 x 80 and
    50 x 50 cells with 10, 0, 33 and 72 agents: tests/scan_cases.handmade_poses"""
    p, layout = SC.handmade_params(pkg, k)
    env = _env(hip, p, 16, scan_obs=True, device_plugins=False, gaze=None, grid_layout=layout)
    size, n, _ = SC.HANDMADE[k]
    assert (env.cfg.W, env.cfg.H, env.cfg.N, env.cfg.grid_tile) == (size[0] // 10, size[1] // 10, n, 16 if layout == 'tiled' else 0)
    alone, kinds = SC.run_handmade(env, lambda: hip.scan_update(env.cfg, env._st, env._scan))
    assert alone == 2 and kinds[0] >= 2 * env.cfg.R and kinds[1] > 0 and kinds[3] > 0 and (kinds[2] >= 2 * env.cfg.R) == (n >= 2)


@pytest.mark.parametrize('name', list(SC.SPECIAL))
def test_the_crowd_and_the_ring_through_the_launch_alone(pkg, hip, name):
    """the crowd: 16 envs of 63, 64, 65 and 72 candidates among 72 agents -- the LDS list one short of its capacity, exactly full
    (the `slot < D2D_SCAN_CCAP` guard at 64, the second ballot pass filling slots up to 63) and overflowing (the kernel tests every
    agent from global memory, cidx == nullptr); the ring: agents centred 0 .. 16 px beyond radius + depth along ray directions,
    either side of the cull bound.  Poisoned buffers, the model without a cull of its own, a second launch that changes nothing"""
    p, layout = SC.SPECIAL[name][0](pkg)
    env = _env(hip, p, 16, scan_obs=True, device_plugins=False, gaze=None, grid_layout=layout)
    assert (env.cfg.W, env.cfg.H, env.cfg.N, env._scan.hit_words) == (50, 50, p.agent_number, (p.agent_number + 31) // 32)
    alone, kinds = SC.run_special(env, name, lambda: hip.scan_update(env.cfg, env._st, env._scan))
    assert alone == 0 and sum(kinds) == 16 * env.cfg.R and kinds[2] > 0 and kinds[3] > 0


# ---------------------------------------------------------------------------------------------------------------- 3. config 5
@pytest.mark.parametrize('layout', ['rowmajor', 'tiled'])
def test_config_5_geometry(pkg, hip, layout):
    """640 x 640 cells, 640 rays (ten lane passes), 100 agents (four hit words), 4 envs, 3 steps; the drones are put next to an
    agent, into an agent and into the far corner, so that the rays meet agents, walls and the range"""
    B = 4
    p = pkg.Params(planner='NoMove', agent_number=100, agent_radius=15, agent_max_speed=40, map_size=[6400, 6400], init_pos=[3200, 3200],
                   target_list=[[6000, 6000]], map_id=50)
    env = _env(hip, p, B, scan_obs=True, device_plugins=False, gaze=None, grid_layout=layout, worlds='device')
    assert (env.cfg.W, env.cfg.H, env.cfg.R, env._scan.hit_words, env.cfg.grid_tile) == (640, 640, 640, 4, 16 if layout == 'tiled' else 0)
    kinds = np.zeros(4, dtype=np.int64)
    for t in range(3):
        ag = env.state.agents.cpu().numpy()
        for e in range(B):
            k = 40 + 7 * e + t
            x, y = round(float(ag[e, A.A_PX, k])), round(float(ag[e, A.A_PY, k]))
            pose = [(x - 30.0, float(y), 0.0), (float(x), float(y), 90.0), (6394.0, 6393.0, 315.0), (3.0, 3200.0 + e, 180.0)][(e + t) % 4]
            env.state.drone[e, :3] = torch.tensor(pose, dtype=torch.float64)
        env.step(torch.zeros(B, dtype=torch.float64))
        env.sync()
        gt = env.state.gt.cpu().numpy().reshape(B, -1)
        for e in range(B):
            got = SC.scan_of(env, e)
            end, kind, hit, obs = SN.scan(env.scan['pose'][e].cpu().numpy(), env.state.agents[e].cpu().numpy(), gt[e], env.cfg, 4, far=True)
            assert got['last_step'] == t + 1 and np.array_equal(got['kind'], kind), (t, e)
            assert np.array_equal(SC.bits(got['end']), SC.bits(end)) and np.array_equal(got['hit'], hit), (t, e)
            assert np.array_equal(SC.bits(got['obs']), SC.bits(obs)), (t, e)
            kinds += np.bincount(kind, minlength=4)
    assert kinds[1] > 0 and kinds[2] > 640 and kinds[3] > 640, kinds


# ---------------------------------------------------------------------------------------------------------------- 4. random soak
def test_random_soak_against_the_model_and_the_fused_steps_union(pkg, hip):
    """16 device-built worlds x 40 steps, 30 agents at speed 40 and radius 10, random actions, against the model; env 5's drone is put
    on the map's edge in front of step 6 (no ray takes a sample, and the collision ends its episode).  The union of a step's hit
    words over the rays equals state.hit of the fused step for every env that stepped: the scan and the step's own raycast are two
    implementations of one.  Coverage, not tolerance: envs that finished and stayed as they ended, and rays of every kind"""
    B, T = 16, 40
    p = pkg.Params(planner='Primitive', agent_number=30, agent_radius=10, agent_max_speed=40, drone_max_speed=40, map_id=3000, max_flight_time=3)
    env = _env(hip, p, B, scan_obs=True, worlds='device')
    cfg, hw = env.cfg, env._scan.hit_words
    gen = torch.Generator().manual_seed(17)
    want = dict(end=np.zeros((B, cfg.R, 2)), kind=np.zeros((B, cfg.R), dtype=np.uint8), hit=np.zeros((B, cfg.R, hw), dtype=np.uint32),
                obs=np.zeros((B, 2, cfg.R), dtype=np.float32), last_step=np.zeros(B, dtype=np.int32))
    kinds, frozen, unions = np.zeros(4, dtype=np.int64), 0, 0
    for t in range(T):
        if t == 5:
            env.state.drone[5, A.D_X] = 0.0
        before = env.state.counters[:, A.C_STEPS].cpu().numpy().copy()
        _step(env, torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1)
        env.sync()
        steps, pose = env.state.counters[:, A.C_STEPS].cpu().numpy(), env.scan['pose'].cpu().numpy()
        agents, gt, union = env.state.agents.cpu().numpy(), env.state.gt.cpu().numpy().reshape(B, -1), env.state.hit.cpu().numpy()
        for e in range(B):
            if steps[e] == before[e]:              # finished: every launch left it alone
                frozen += 1
                continue
            want['end'][e], want['kind'][e], want['hit'][e], want['obs'][e] = SN.scan(pose[e], agents[e], gt[e], cfg, hw, far=True)
            want['last_step'][e] = steps[e]
            kinds += np.bincount(want['kind'][e], minlength=4)
            assert np.array_equal(SC.unpack(np.bitwise_or.reduce(want['hit'][e], axis=0), cfg.N), union[e]), (t, e)
            unions += 1
        got = {k: env.scan[k].cpu().numpy() for k in want}
        got['hit'] = got['hit'].view(np.uint32)
        for k in want:
            assert np.array_equal(SC.bits(got[k]), SC.bits(want[k])), (t, k, np.argwhere(SC.bits(got[k]) != SC.bits(want[k]))[:5].tolist())
    assert bool(env.state.flags[:, A.F_DONE].all()) and frozen > B and unions > 10 * B and kinds.min() > 0, (frozen, unions, kinds)


# ---------------------------------------------------------------------------------------------------------------- 5. the stream
@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Primitive-RVO', 'Jerk-CVM'])
def test_a_stream_with_the_channel_equals_the_stream_without(pkg, hip, cell):
    """8 slots, 24 episodes, a turn every 4 steps; a refilled slot shows the cleared channel at its step 0"""
    slots, M = 8, 24
    p = AC.params_of(pkg, cell)
    refills, frozen = SC.stream_pair(lambda q, n, scan: _env(hip, q, n, scan_obs=scan, worlds='device'), p, slots, M)
    assert refills == M - slots and frozen > 0


def test_the_library_refuses_what_it_cannot_hold(pkg, hip):
    import copy
    import ctypes as C
    env = _env(hip, AC.params_of(pkg, 'Primitive-CVM'), 1, scan_obs=True)
    hip.scan_update(env.cfg, env._st, env._scan)
    big = copy.copy(env.cfg)
    big.W, big.H = 32767 * 3, 32767
    assert hip.yfn['update'](C.byref(big), C.byref(env._st), C.byref(env._scan), None) == -4
    assert b'32-bit indices' in hip.yfn['last_error']()
    assert hip.yfn['update'](C.byref(env.cfg), C.byref(env._st), None, None) == -1
    SC.check_cleared(env, 0)                       # the launch over a world that has not stepped wrote nothing
