"""The recorded Jerk_Primitive worlds (tests/golden/jerk_traces.npz, written by tests/golden/make_jerk_golden.py) for the tests that
replay them: the scene plan() saw at every step, for the model; and the episode through a VecDrone2DEnv or a Drone2DEnv2, for the
env tests on the oracle (test_jerk_env_cpu.py) and on the device (test_gpu_jerk_env.py)."""
import functools
import json
import os

import numpy as np

import jerk_model as M

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jerk_traces.npz')


@functools.lru_cache(maxsize=None)
def traces():
    return dict(np.load(PATH))


def world_names():
    return [str(n) for n in traces()['names']]


def world(i):
    z = traces()
    pre = f'w{i}_'
    w = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
    w['cfg'] = json.loads(str(w['cfg']))
    return w


def tie_table():
    z = traces()
    return z['tie_perm'], z['tie_eq']


def params_of(pkg, w, **kw):
    return pkg.Params(**dict(dict(planner='Jerk_Primitive', gaze_method='NoControl'), **dict(w['cfg'], **kw)))


def scene(pkg, w, t):
    """what plan() saw at step t of recorded world w, as tests/jerk_model.py reads it"""
    p = params_of(pkg, w)
    W, H = p.map_size[0] // p.map_scale, p.map_size[1] // p.map_scale
    wall = np.unpackbits(w['t_p_wall'][t])[:W * H].reshape(W, H)
    N = int(w['N'])
    return dict(drone=tuple(w['t_p_drone'][t]), target=tuple(w['t_p_target'][t]), dmap=np.where(wall, 1, 2).astype(np.uint8),
                trackers=[(w['t_p_mu'][t][k], w['t_p_radius'][t][k]) for k in range(N) if w['t_p_active'][t][k]],
                scale=p.map_scale, map_size=tuple(p.map_size), drone_radius=p.drone_radius, var_cam=p.var_cam, v_max=p.drone_max_speed,
                dt=p.dt)


def check_step(w, t, state, jerk, e=0, kf_tol=1e-6):
    """every recorded field of step t of world w against env e of a VecDrone2DEnv's state after that step"""
    from drone2d_amd import _abi as A
    d = state.drone[e].cpu().numpy()
    c = state.counters[e].cpu().numpy()
    f = state.flags[e].cpu().numpy()
    assert int(state.plan_ok[e]) == int(w['t_plan_ok'][t]) == int(state.wp_valid[e]), t
    assert int(jerk.t['choice'][e]) == int(w['t_choice'][t]), t
    assert M.bits_equal(state.wp[e].cpu().numpy(), w['t_wp'][t]), t
    assert M.bits_equal(d[[A.D_X, A.D_Y, A.D_YAW]], w['t_drone'][t]), t
    assert M.bits_equal(d[[A.D_VX, A.D_VY, A.D_AX, A.D_AY]], w['t_vel'][t]), t
    assert int(c[A.C_SM]) == int(w['t_sm'][t]) and int(c[A.C_FAIL]) == int(w['t_fail'][t]), t
    assert f[:3].tolist() == w['t_flags'][t].tolist() and bool(f[A.F_DONE]) == bool(w['t_done'][t]), t
    assert bool(int(jerk.t['stat'][e]) & A.JERK_STAT_TIE) == bool(w['t_tie'][t]), t
    assert not int(jerk.t['stat'][e]) & A.JERK_STAT_UNKNOWN, t
    N = int(w['N'])
    if N:                                                   # the trackers plan() saw: those of the end of the step
        mu = state.kf[e, :N, :4].cpu().numpy()
        act = state.active[e, :N].cpu().numpy().astype(bool)
        assert np.array_equal(act, w['t_p_active'][t].astype(bool)), t
        assert np.allclose(mu[act], w['t_p_mu'][t][act], rtol=0, atol=kf_tol), t


def replay_vec(pkg, backend, i, B=1, reset_at=None, T=None):
    """world i through VecDrone2DEnv(planner='Jerk_Primitive', device_plugins=True) with the recorded tie table, every env of the
    batch the same world; `reset_at`: after that many steps the batch is reset and the episode replays from its start"""
    import torch
    from drone2d_amd import vec_env
    w = world(i)
    p = params_of(pkg, w)
    worlds = [vec_env.build_worlds(p, 1)[0]] * B
    env = vec_env.VecDrone2DEnv(p, B, backend=backend, planner='Jerk_Primitive', device_plugins=True, gaze='external', worlds=worlds,
                                jerk_tie=tie_table())
    T = len(w['t_done']) if T is None else min(T, len(w['t_done']))
    if reset_at is not None:
        for t in range(reset_at):
            env.step(np.full(B, w['actions'][t]))
        env.reset(torch.ones(B, dtype=torch.uint8) if B > 1 else None)
    for t in range(T):
        env.step(np.full(B, w['actions'][t]))
        for e in sorted({0, B - 1}):
            check_step(w, t, env.state, env.jerk, e)
    return env
