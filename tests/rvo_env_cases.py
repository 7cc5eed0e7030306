"""What the RVO env tests run, on whichever backend they are given: the HIP library on the GPU (test_gpu_rvo_env.py), or the CPU
oracle with the host build of csrc/rvo/d2d_rvo.h (rvo_backend.OracleRvoBackend, test_rvo_env_cpu.py)."""
import json

import numpy as np
import torch

import replay
import rvo_cases as RC
import rvo_model as M


class _Prefixed:
    """the `full_` arrays of a recorded world under the names tests/replay.py reads"""

    def __init__(self, w):
        self.d = {k[len('full_'):]: v for k, v in w.items() if k.startswith('full_')}
        self.d.update({k: w[k] for k in ('t_agent_pos', 't_agent_pref', 't_done')})
        self.files = list(self.d)

    def __getitem__(self, k):
        return self.d[k]


def params_of(pkg, w):
    return replay.params_from(w, pkg)


def agents_equal(env, e, pos, vel, pref):
    ag = env.state.agents[e].cpu().numpy()
    v = env.state.agent_vel[e].cpu().numpy()
    return M.bits_equal(ag[0:2].T, pos) and M.bits_equal(ag[2:4].T, pref) and M.bits_equal(v.T, vel)


def step_world(pkg, backend, i, worlds=None, copies=1):
    """VecDrone2DEnv(motion_profile='RVO').step through recorded world i: the agents everywhere, the other step outputs where stored"""
    from drone2d_amd import vec_env
    w = RC.world(i)
    p = params_of(pkg, w)
    assert p.motion_profile == 'RVO'
    if worlds is None and copies > 1:                                 # `copies` envs of the one recorded world, not its neighbours' seeds
        from drone2d_amd import host_init
        worlds = [host_init.init_world(p)] * copies
    env = vec_env.VecDrone2DEnv(p, copies, backend=backend, worlds=worlds, grid_layout='rowmajor')
    assert env.rvo and M.bits_equal(env.state.agent_vel[0].cpu().numpy().T, w['agent_vel'])
    full = 'full_t_action' in w
    cmp = None
    if full:
        cmp = replay.Replay.__new__(replay.Replay)
        cmp.A, cmp.fx, cmp.name, cmp.cfg, cmp.st = pkg._abi, _Prefixed(w), RC.world_names()[i], env.cfg, env.state
    for t in range(len(w['t_done'])):
        env.step(np.full(copies, float(w['full_t_action'][t]) if full else 0.0))
        env.sync()
        for e in {0, copies - 1}:
            assert agents_equal(env, e, w['t_agent_pos'][t], w['t_agent_vel'][t], w['t_agent_pref'][t]), (RC.world_names()[i], t, e)
            if full:
                cmp.compare(t, e)
    return env


def soak(pkg, backend, reference, B=8, T=25, seed=5):
    """B seeded envs x T steps with random actions on `backend` and on `reference` (the CPU oracle + the host loops, themselves held
    to the Python model): every state field, bit for bit; and the Python model itself on the agents of every env"""
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=7, agent_radius=12, agent_max_speed=30, pillar_number=3, map_id=40)
    worlds = vec_env.build_worlds(p, B)
    dev = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds, grid_layout='rowmajor')
    ref = vec_env.VecDrone2DEnv(p, B, backend=reference, worlds=worlds, grid_layout='rowmajor')
    model = {e: (worlds[e]['agents'][0:2].T.copy(), np.zeros((7, 2)), worlds[e]['agents'][2:4].T.copy()) for e in range(B)}
    rng = np.random.RandomState(seed)
    for t in range(T):
        a = rng.uniform(-1, 1, B)
        dev.step(a)
        ref.step(a)
        dev.sync()
        for name in ('agents', 'agent_vel', 'gt', 'dmap', 'drone', 'flags', 'hit', 'obs_local', 'counters', 'kf', 'active'):
            assert torch.equal(dev.state.t[name].cpu(), ref.state.t[name].cpu()), (t, name)
        for e, (pos, vel, pref) in model.items():
            model[e] = M.step_world(pos, vel, pref, worlds[e]['agents'][4], worlds[e]['obstacles'])
            assert agents_equal(dev, e, *model[e]), (t, e)


def rollout_equals_steps(pkg, backend, T=6, B=3):
    from drone2d_amd import vec_env
    A = pkg._abi
    p = pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=9, agent_radius=15, agent_max_speed=20, map_id=3)
    worlds = vec_env.build_worlds(p, B)
    one = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds)
    many = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds)
    rng = np.random.RandomState(1)
    acts = rng.uniform(-1, 1, (T, B))
    a0 = worlds[0]['agents']
    pin = np.array([[a0[0, 0] + 3, a0[1, 0] + 2], [250.0, 250.0], [120.0, 400.0]])[:B]       # env 0: on top of its first agent
    coll = one.rollout(acts, pin=pin, collisions=True, streams=2)
    want = []
    for t in range(T):
        many.state.drone[:, A.D_X:A.D_Y + 1] = torch.as_tensor(pin, device=many.device)
        many.step(acts[t])
        want.append(many.state.flags[:, A.F_COLLISION].cpu().clone())
    one.sync()
    assert torch.equal(coll.cpu(), torch.stack(want)) and int(coll[:, 0].max()) == 2
    for name in ('agents', 'agent_vel', 'gt', 'dmap', 'drone', 'flags', 'counters', 'kf'):
        assert torch.equal(one.state.t[name].cpu(), many.state.t[name].cpu()), name


def rollout_draws_a_noise_row_per_step(pkg, backend, T=12, B=3):
    """var_cam != 0 with a [T, B, N, 2] block of draws: step t of a rollout takes row t, also when the run is cut into two calls --
    held to T calls of set_noise(row t) + step.  The drone is pinned among the agents so that rays hit them and the rows matter."""
    from drone2d_amd import vec_env
    A = pkg._abi
    p = pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=25, agent_radius=10, agent_max_speed=20, map_id=11, var_cam=2)
    worlds = vec_env.build_worlds(p, B)
    for w in worlds:
        w.pop('rng', None)                                   # the caller supplies the draws (set_noise)
    rng = np.random.RandomState(2)
    noise, acts = rng.standard_normal((T, B, 25, 2)), rng.uniform(-1, 1, (T, B))
    pin = np.full((B, 2), 250.0)
    one = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds)
    many = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds)
    one.set_noise(noise)
    one.rollout(acts[:5], pin=pin)
    one.rollout(acts[5:], pin=pin)
    hits = 0
    for t in range(T):
        many.set_noise(noise[t])
        many.state.drone[:, A.D_X:A.D_Y + 1] = torch.as_tensor(pin, device=many.device)
        many.step(acts[t])
        hits += int(many.state.hit.sum())
    one.sync()
    assert hits > 0 and bool(many.state.active.any())
    for name in ('agents', 'agent_vel', 'kf', 'kf_len', 'active', 'gt', 'dmap', 'counters'):
        assert torch.equal(one.state.t[name].cpu(), many.state.t[name].cpu()), name
    # the rows matter: the same run on row 0 alone ends elsewhere
    same = vec_env.VecDrone2DEnv(p, B, backend=backend, worlds=worlds)
    same.set_noise(noise[0])
    same.rollout(acts, pin=pin)
    same.sync()
    assert not torch.equal(same.state.kf.cpu(), one.state.kf.cpu())


def reset_restores_masked_velocities(pkg, backend, B=4):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=6, agent_radius=10, agent_max_speed=20, map_id=9,
                   static_map='maps/obstacle_map.npy')
    env = vec_env.VecDrone2DEnv(p, B, backend=backend)
    vel0, ag0 = env.state.agent_vel.cpu().clone(), env.state.agents.cpu().clone()
    assert not vel0[:, :, :6].any() and torch.equal(vel0[:, :, 6:], ag0[:, 2:4, 6:]) and vel0[:, :, 6:].any()
    for _ in range(3):
        env.step(np.zeros(B))
    env.sync()
    moved_v, moved_a = env.state.agent_vel.cpu().clone(), env.state.agents.cpu().clone()
    assert not torch.equal(moved_v[:, :, :6], vel0[:, :, :6])
    mask = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
    env.reset(mask)
    env.sync()
    v, a = env.state.agent_vel.cpu(), env.state.agents.cpu()
    for e in range(B):
        assert torch.equal(v[e], vel0[e] if mask[e] else moved_v[e]) and torch.equal(a[e], ag0[e] if mask[e] else moved_a[e]), e
    env.reset()
    env.sync()
    assert torch.equal(env.state.agent_vel.cpu(), vel0)


def episode(pkg, backend, device):
    """Drone2DEnv2 + Experiment through the recorded Primitive + LookAhead episode under RVO: the policy's action of every step (this
    package's host LookAhead), the flags and the CSV row"""
    from drone2d_amd import runner, gaze, env as envmod
    fx = RC.fixture()
    kw = json.loads(str(fx['ep_cfg']))
    p = pkg.Params(debug=True, motion_profile='RVO', **kw)
    p.render = False
    env = envmod.Drone2DEnv2(p, device=device, backend=backend)
    pol = gaze.policy_list[kw['gaze_method']](p)
    acts, done, info = [], False, None
    while not done and len(acts) <= len(fx['ep_actions']):
        a = pol.plan(env.info)
        acts.append(float(a))
        _, _, done, info = env.step(a)
    assert np.array_equal(np.array(acts), fx['ep_actions'])
    want = fx['ep_row']
    assert [info['collision_flag'] == 1, info['collision_flag'] == 2, info['freezing_flag'], info['dead_lock_flag']] == list(want[5:9])
    vel = np.array([ag.velocity for ag in env.agents])                   # AgentProxy.velocity: what RVO_update assigned
    assert M.bits_equal(vel, env._vec.state.agent_vel[0].cpu().numpy().T)
    assert not M.bits_equal(vel, np.array([ag.pref_velocity for ag in env.agents]))
    row = runner.Experiment(p, device=device, backend=backend).run()
    got = np.array([float(x) for x in row[12:]], dtype=np.float64)
    assert row[2] == 'RVO' and np.allclose(got, want, rtol=0, atol=1e-9, equal_nan=True), (got, want)


def cvm_next_to_rvo(pkg, backend):
    """a CVM env built next to an RVO env still equals its own fixture"""
    from drone2d_amd import vec_env
    rvo = vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', motion_profile='RVO', agent_number=10, agent_radius=15, agent_max_speed=20,
                                           map_id=1), 2, backend=backend)
    rvo.step(np.zeros(2))
    r = replay.Replay(pkg, backend, 'nomove_n10_rand_map2')
    r.run('fused', every=7)
    rvo.step(np.zeros(2))
    rvo.sync()
    cvm = vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1), 1, backend=backend)
    assert not cvm.rvo and 'agent_vel' not in cvm.state.t
