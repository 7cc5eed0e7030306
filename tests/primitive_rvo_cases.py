"""The recorded Primitive episodes under the RVO motion profile (tests/golden/primitive_rvo_episodes.npz, written by
tests/golden/make_primitive_rvo_golden.py) for the tests that replay them through runner.SteppedExperimentBatch /
VecDrone2DEnv.run_episodes: on the oracle with the host RVO build (test_primitive_rvo_episodes_cpu.py, the worlds whose gaze policy the
oracle has) and on the device (test_gpu_primitive_rvo_episodes.py, every world).  Test infrastructure."""
import copy
import functools
import json
import os

import numpy as np

from drone2d_amd import _abi as A
from jerk_gaze_cases import bits_equal, check_row   # noqa: F401  (check_row: columns 12 .. 21, its column-15 rule included)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'primitive_rvo_episodes.npz')
SCRATCH = ('nodes', 'hash', 'launch_args')      # plugin buffers whose contents mean nothing between calls
ORACLE_GAZE = ('Oxford', 'Rotating', 'NoControl')


@functools.lru_cache(maxsize=None)
def traces():
    return dict(np.load(PATH))


def world_names():
    return [str(n) for n in traces()['names']]


@functools.lru_cache(maxsize=None)
def world(i):
    z = traces()
    pre = f'w{i}_'
    w = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
    w['cfg'] = json.loads(str(w['cfg']))
    return w


def params_of(pkg, w, **kw):
    return pkg.Params(**dict(dict(planner='Primitive'), **dict(w['cfg'], **kw)))


def backend_of(backend):
    """`backend` itself, or for the string 'oracle' a fresh tests/stepped_backend.SteppedOracleBackend (one per env: see there)"""
    if backend == 'oracle':
        from stepped_backend import SteppedOracleBackend
        return SteppedOracleBackend()
    return backend


def attach(backend, env):
    if hasattr(backend, 'attach'):
        backend.attach(env)
    return env


def batch_of(pkg, backend, p, B=1, **kw):
    from drone2d_amd import runner
    backend = backend_of(backend)
    xb = runner.SteppedExperimentBatch(p, B, device=str(getattr(backend, 'device', 'cpu')), backend=backend, **kw)
    attach(backend, xb.env)
    return xb


def env_of(pkg, backend, p, B, gaze, **kw):
    from drone2d_amd import vec_env
    backend = backend_of(backend)
    return attach(backend, vec_env.VecDrone2DEnv(p, B, backend=backend, planner='Primitive', device_plugins=True, gaze=gaze, **kw))


def check_step(w, t, env, e=0):
    """every recorded field of step t of world w against env e of a VecDrone2DEnv after that step, bit for bit"""
    s = env.state
    d = s.drone[e].cpu().numpy()
    c = s.counters[e].cpu().numpy()
    f = s.flags[e].cpu().numpy()
    assert bits_equal(float(s.action[e]), w['t_action'][t]), (t, float(s.action[e]), float(w['t_action'][t]))
    if 't_owl_U' in w:
        owl = env.plugins.t['owl_state'][e].cpu().numpy()
        assert bits_equal(owl[:A.OWL_NDIR], w['t_owl_U'][t]), t
        assert owl[A.OWL_S_LEFT] == w['t_owl_left'][t] and bits_equal(owl[A.OWL_S_RATE], w['t_owl_rate'][t]), t
    assert int(s.plan_ok[e]) == int(w['t_plan_ok'][t]), t
    assert int(s.wp_valid[e]) == int(w['t_wp_valid'][t]), t
    if w['t_wp_valid'][t]:
        assert bits_equal(s.wp[e].cpu().numpy(), w['t_wp'][t]), t
    hdr = env.plugins.t['traj_hdr'][e].cpu().numpy()
    assert int(hdr[1] - hdr[0]) == int(w['t_traj_len'][t]), (t, hdr.tolist(), int(w['t_traj_len'][t]))
    assert bits_equal(d[[A.D_X, A.D_Y, A.D_YAW]], w['t_drone'][t]), t
    assert bits_equal(d[[A.D_VX, A.D_VY, A.D_AX, A.D_AY]], w['t_vel'][t]), t
    assert int(c[A.C_SM]) == int(w['t_sm'][t]) and int(c[A.C_FAIL]) == int(w['t_fail'][t]), t
    assert f[:3].tolist() == w['t_flags'][t].tolist() and bool(f[A.F_DONE]) == bool(w['t_done'][t]), t
    N = int(w['N'])
    ag = s.agents[e].cpu().numpy()
    assert bits_equal(ag[[A.A_PX, A.A_PY], :N].T, w['t_agent_pos'][t]), t
    assert bits_equal(s.agent_vel[e].cpu().numpy()[:, :N].T, w['t_agent_vel'][t]), t


def frozen_snapshot(env, e):
    """everything of env e that a step may write: the whole state (its agents and their velocities included) and the plugin state"""
    env.sync()
    out = {'s.' + k: v[e].cpu().clone() for k, v in env.state.t.items() if k != 'agent_vel_out'}
    out.update({'p.' + k: v[e].cpu().clone() for k, v in env.plugins.t.items() if k not in SCRATCH})
    return out


def same_frozen(a, b):
    import torch
    return [k for k in a if not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))] == []


def replay(pkg, backend, i):
    """world i, step for step through run_episodes(max_steps=1), then frozen over three more steps; and in one run() of a fresh
    batch: the same row and the same final state"""
    w = world(i)
    p = params_of(pkg, w)
    xb = batch_of(pkg, backend, p)
    env = xb.env
    T = len(w['t_done'])
    assert xb.params.gaze_method == w['cfg']['gaze_method'] == env.step_gaze and env.rvo and env.jerk is None
    for t in range(T):
        assert env.run_episodes(max_steps=1) == 1
        check_step(w, t, env)
    assert bool(env.state.flags[0, A.F_DONE])
    end = frozen_snapshot(env, 0)
    assert env.run_episodes(max_steps=3) == 3
    assert same_frozen(end, frozen_snapshot(env, 0))
    check_row(w, xb.rows()[0])
    whole = batch_of(pkg, backend, p)
    rows = whole.run(check_every=16)
    assert all((a != a and b != b) or a == b for a, b in zip(rows[0], xb.rows()[0]))
    assert T <= whole.steps_run <= min(whole.max_steps, (T + 15) // 16 * 16)
    assert same_frozen(end, frozen_snapshot(whole.env, 0))
    return xb


def staggered(pkg, backend, p, B=3):
    """a B-env batch whose envs end at different steps: everything of an env stays bit-equal from its terminal step over five steps
    past the last env's end, and the rows equal B one-env runs"""
    xb = batch_of(pkg, backend, p, B=B)
    env = xb.env
    ended, snaps = {}, {}
    for t in range(xb.max_steps):
        env.run_episodes(max_steps=1)
        done = env.state.flags[:, A.F_DONE].cpu().numpy()
        for e in range(B):
            if done[e] and e not in ended:
                ended[e], snaps[e] = t, frozen_snapshot(env, e)
        if len(ended) == B:
            break
    assert len(ended) == B and len(set(ended.values())) == B, ended
    env.run_episodes(max_steps=5)
    for e in range(B):
        assert same_frozen(snaps[e], frozen_snapshot(env, e)), e
    rows = xb.rows()
    for e in range(B):
        q = copy.copy(p)
        q.map_id = p.map_id + e
        one = batch_of(pkg, backend, q, B=1)
        r = one.run()[0]
        assert one.steps_run >= ended[e] + 1
        assert all((a != a and b != b) or a == b for a, b in zip(r, rows[e])), (e, r, rows[e])
    return ended


def cvm_equals_closed_loop(pkg, backend, B, gaze='Oxford', steps=None, **kw):
    """under CVM run_episodes() on the Primitive plugins is closed_loop(freeze_done=True): every state and plugin field after the
    episodes, and the steps in between for a few of them"""
    import torch
    p = pkg.Params(**dict(dict(planner='Primitive', gaze_method=gaze, agent_number=10, agent_radius=15, agent_max_speed=20,
                               drone_max_speed=40, max_flight_time=8, map_id=0, target_list=[[50, 230]]), **kw))
    a, b = (env_of(pkg, backend, p, B, gaze) for _ in range(2))
    n = int(np.ceil(p.max_flight_time / p.dt)) + 1 if steps is None else steps
    done_at = []
    for chunk in (1, 7, n - 8):
        assert a.run_episodes(max_steps=chunk) == chunk
        b.closed_loop(chunk, freeze_done=True)
        sa, sb = ({**{'s.' + k: v for k, v in e.state.t.items()}, **{'p.' + k: v for k, v in e.plugins.t.items() if k not in SCRATCH}}
                  for e in (a, b))
        a.sync(), b.sync()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (chunk, k)
        done_at.append(int(a.state.flags[:, A.F_DONE].sum()))
    assert done_at[-1] == B and len(set(a.state.counters[:, A.C_STEPS].tolist())) > 1, done_at
    return a
