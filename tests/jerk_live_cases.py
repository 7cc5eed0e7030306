"""Whole Jerk_Primitive episodes with every launch leaving finished envs alone (VecDrone2DEnv.run_episodes(live=...),
include/d2d_jerk_live.h): the checks that test_jerk_live_cpu.py runs on tests/jerk_live_backend.LiveJerkBackend and
test_gpu_jerk_live_episodes.py on the device.  Test infrastructure.

`backend` is a backend object shared by every env (the HIP backend), or a class of which every env gets an instance of its own that
is told about the env (`attach`: see tests/jerk_live_backend.py)."""
import copy

import numpy as np

from drone2d_amd import _abi as A
import jerk_gaze_cases as EC

CVM_MAP_ID = 20      # as test_gpu_jerk_episodes.py: maps 20, 21, 22 end at three different steps
RVO_MAP_ID = 0       # maps 0, 1, 2 under RVO end after 102, 111 and 101 steps (test_jerk_live_cpu.py searches 0, 3, 6 ... on the CPU)

# Every tensor with a leading env dimension of the state, the planner's own state and the Owl state is compared, but this one.  It is
# per env, yet no state: the two velocity buffers swap after each RVO step, agent_vel is then the velocity and agent_vel_out the
# buffer the next decision launch overwrites.  A loop that stops at an env's terminal step leaves the velocity of the step before in
# it; one masked launch later it holds a copy of agent_vel (that copy is how the swap keeps a finished env's velocity).  Its
# contents therefore say how many launches ran after the env ended, which differs between a batch and a one-env run by design.
SCRATCH = ('s.agent_vel_out',)


def params(pkg, profile, map_id, **kw):
    return pkg.Params(**dict(dict(planner='Jerk_Primitive', gaze_method='Owl', motion_profile=profile, agent_number=10, agent_radius=15,
                                  agent_max_speed=20, drone_max_speed=40, max_flight_time=12, map_id=map_id), **kw))


def env_of(pkg, backend, p, B, **kw):
    from drone2d_amd import vec_env
    if isinstance(backend, type):
        backend = backend()
    env = vec_env.VecDrone2DEnv(p, B, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze=p.gaze_method,
                                jerk_tie=EC.tie_table(), **kw)
    if hasattr(backend, 'attach'):
        backend.attach(env)
    return env


def buffers(env):
    """name -> tensor of everything the env holds per env: state.t, jerk.t and the Owl state, taken from the objects"""
    out = {'s.' + k: v for k, v in env.state.t.items()}
    out.update({'j.' + k: v for k, v in env.jerk.t.items()})
    if env.gaze_state is not None and env.gaze_state.owl_state is not None:
        out['g.owl_state'] = env.gaze_state.owl_state
    assert all(v.shape[0] == env.num_envs for v in out.values()), {k: tuple(v.shape) for k, v in out.items()}
    for k in ('s.agents', 's.drone', 's.counters', 's.flags', 's.gt', 's.dmap', 's.kf', 's.active', 's.action', 's.plan_ok', 's.wp_valid',
              's.wp', 's.hit', 's.obs_local', 'j.choice', 'j.stat', 'j.trk_radius', 'j.trk_prev'):
        assert k in out, k
    if env.rvo:
        assert 's.agent_vel' in out and 's.agent_vel_out' in out
    return {k: v for k, v in out.items() if k not in SCRATCH}


def snapshot(env, e):
    env.sync()
    return {k: v[e].cpu().clone() for k, v in buffers(env).items()}


def differing(a, b):
    import torch
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))]


def steps_played(env):
    env.sync()
    assert bool(env.state.flags[:, A.F_DONE].all())
    return env.state.counters[:, A.C_STEPS].tolist()


def a_finished_env_is_its_own_single_env_episode(pkg, backend, p, B=3, **run):
    """the batch to its end, then each env alone with check_every=1 (that loop stops at the env's terminal step): every buffer equal"""
    env = env_of(pkg, backend, p, B)
    env.run_episodes(**run)
    ended = steps_played(env)
    assert len(set(ended)) == B, ended
    bad = {}
    for e in range(B):
        q = copy.copy(p)
        q.map_id = p.map_id + e
        one = env_of(pkg, backend, q, 1)
        assert one.run_episodes(check_every=1, **run) == ended[e] == steps_played(one)[0]
        diff = differing(snapshot(env, e), snapshot(one, 0))
        if diff:
            bad[e] = diff
    assert not bad, bad
    return ended


def frozen_from_the_terminal_step_on(pkg, backend, p, B=3, **run):
    env = env_of(pkg, backend, p, B)
    n = int(np.ceil(p.max_flight_time / p.dt)) + 1
    ended, snaps = {}, {}
    for t in range(n):
        env.run_episodes(max_steps=1, **run)
        done = env.state.flags[:, A.F_DONE].cpu().numpy()
        for e in range(B):
            if done[e] and e not in ended:
                ended[e], snaps[e] = t, snapshot(env, e)
        if len(ended) == B:
            break
    assert len(ended) == B and len(set(ended.values())) == B, ended
    assert env.run_episodes(max_steps=5, **run) == 5
    bad = {e: differing(snaps[e], snapshot(env, e)) for e in range(B)}
    assert not any(bad.values()), bad
    return ended


def masked_equals_unmasked(pkg, backend, profile, gaze, B=64, early=10):
    """live=True against live=False: after `early` steps every buffer of the envs not yet done, at the end every CSV row"""
    from drone2d_amd import runner
    p = params(pkg, profile, 0, gaze_method=gaze, max_flight_time=8, target_list=[[50, 230]])
    xb = [runner.SteppedExperimentBatch(p, B, device=str(getattr(backend, 'device', 'cpu')), backend=backend, jerk_tie=EC.tie_table())
          for _ in range(2)]
    for x, live in zip(xb, (True, False)):
        assert x.env.run_episodes(max_steps=early, live=live) == early
    snaps = [{k: v.cpu() for k, v in buffers(x.env).items()} for x in xb]
    going = ~xb[0].env.state.flags[:, A.F_DONE].bool().cpu()
    assert bool(going.any())
    assert differing(*({k: v[going] for k, v in s.items()} for s in snaps)) == []
    for x, live in zip(xb, (True, False)):
        x.env.run_episodes(live=live)
        x.env.sync()
    ended = steps_played(xb[0].env)
    assert ended == steps_played(xb[1].env) and len(set(ended)) > 3
    rows = [x.rows() for x in xb]
    assert len(rows[0]) == len(rows[1]) == B
    for r, s in zip(*rows):
        assert len(r) == len(s) == 22 and all((a != a and b != b) or a == b for a, b in zip(r, s)), (r, s)
    return ended


def a_masked_reset_starts_fresh_episodes_for_those_envs_alone(pkg, backend, p, B=3):
    import torch
    env = env_of(pkg, backend, p, B)
    env.run_episodes()
    ended = steps_played(env)
    first = [snapshot(env, e) for e in range(B)]
    env.reset(torch.tensor([0, 1, 0], dtype=torch.uint8))
    env.sync()
    assert env.state.flags[:, A.F_DONE].tolist() == [1, 0, 1] and differing(first[1], snapshot(env, 1))
    env.run_episodes()
    assert steps_played(env) == ended
    bad = {e: differing(first[e], snapshot(env, e)) for e in range(B)}
    assert not any(bad.values()), bad
