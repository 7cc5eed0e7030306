"""The recorded Jerk_Primitive episodes (tests/golden/jerk_gaze_episodes.npz, written by tests/golden/make_jerk_gaze_golden.py) for the
tests that replay them: what the reference's gaze policy saw and answered at every step, for the host build of csrc/gaze/d2d_gaze.h
(test_gaze_host_build.py); and the whole episode through runner.SteppedExperimentBatch / VecDrone2DEnv.run_episodes, on the oracle
(test_jerk_episodes_cpu.py) and on the device (test_gpu_jerk_episodes.py).  Test infrastructure."""
import copy
import functools
import json
import os

import numpy as np

from drone2d_amd import _abi as A

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jerk_gaze_episodes.npz')
FROZEN = ('drone', 'counters', 'flags', 'dmap', 'gt', 'kf', 'active', 'action')   # + the Owl state: what "frozen" means


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


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


def tie_table():
    z = traces()
    return z['tie_perm'], z['tie_eq']


def params_of(pkg, w, **kw):
    return pkg.Params(**dict(dict(planner='Jerk_Primitive'), **dict(w['cfg'], **kw)))


def policy_inputs(w, t):
    """the arrays of a one-env d2d_gaze_call for the policy call of step t: what the reference's policy saw, the Owl state it held"""
    N = int(w['N'])
    drone = np.zeros((1, A.DF))
    drone[0, [A.D_X, A.D_Y, A.D_YAW, A.D_VX, A.D_VY]] = w['t_g_drone'][t]
    kf = np.zeros((1, N, A.KF))
    owl = np.zeros((1, A.OWL_STATE_F))
    if N:
        kf[0, :, :4] = w['t_g_mu'][t]
    if t and 't_owl_U' in w:
        owl[0, :A.OWL_NDIR], owl[0, A.OWL_S_LEFT], owl[0, A.OWL_S_RATE] = w['t_owl_U'][t - 1], w['t_owl_left'][t - 1], w['t_owl_rate'][t - 1]
    active = np.ascontiguousarray(w['t_g_active'][t].reshape(1, N)) if N else np.zeros((1, 0), np.uint8)
    return dict(drone=drone, target=np.ascontiguousarray(w['t_g_target'][t].reshape(1, 2)), active=active, kf=kf, owl_state=owl)


def check_step(w, t, env, e=0, kf_tol=1e-6):
    """every recorded field of step t of world w against env e of a VecDrone2DEnv after that step.  Everything is held bit for bit
    but the trackers' means, which the reference's Kalman filter computes through BLAS (as tests/jerk_env_cases.py holds them)"""
    s = env.state
    d = s.drone[e].cpu().numpy()
    c = s.counters[e].cpu().numpy()
    f = s.flags[e].cpu().numpy()
    assert bits_equal(float(s.action[e]), w['t_action'][t]), (t, float(s.action[e]), float(w['t_action'][t]))
    if 't_owl_U' in w:
        owl = env.gaze_state.owl_state[e].cpu().numpy()
        assert bits_equal(owl[:A.OWL_NDIR], w['t_owl_U'][t]), t
        assert owl[A.OWL_S_LEFT] == w['t_owl_left'][t] and bits_equal(owl[A.OWL_S_RATE], w['t_owl_rate'][t]), t
    assert int(s.plan_ok[e]) == int(w['t_plan_ok'][t]) == int(s.wp_valid[e]), t
    assert int(env.jerk_choice[e]) == int(w['t_choice'][t]), t
    assert not int(env.jerk_stat[e]) & A.JERK_STAT_UNKNOWN, t
    assert bits_equal(d[[A.D_X, A.D_Y, A.D_YAW]], w['t_drone'][t]), t
    assert bits_equal(d[[A.D_VX, A.D_VY, A.D_AX, A.D_AY]], w['t_vel'][t]), t
    assert int(c[A.C_SM]) == int(w['t_sm'][t]) and int(c[A.C_FAIL]) == int(w['t_fail'][t]), t
    assert f[:3].tolist() == w['t_flags'][t].tolist() and bool(f[A.F_DONE]) == bool(w['t_done'][t]), t
    N = int(w['N'])
    if N and t + 1 < len(w['t_done']):                      # the trackers the NEXT policy call saw: those of the end of this step
        act = s.active[e, :N].cpu().numpy().astype(bool)
        assert np.array_equal(act, w['t_g_active'][t + 1].astype(bool)), t
        assert np.allclose(s.kf[e, :N, :4].cpu().numpy()[act], w['t_g_mu'][t + 1][act], rtol=0, atol=kf_tol), t


def check_row(w, row):
    """columns 12 .. 21 of a CSV row (experiment.py:91-101) against the reference's: equal, but for the mean tracked time.  The
    reference sums len(ts) * 0.1 over the tracked agents and divides; the state keeps the total number of samples, and the row
    assembly runner.batch_rows shares with ExperimentBatch multiplies it by 0.1 once.  The two roundings differ by a few ulps of a
    number below max_flight_time; the column is held to 1e-9, as tests/test_runner.py holds it for ExperimentBatch"""
    got, want = list(row[12:]), w['row'].tolist()
    assert len(got) == len(want) == 10
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a != a and b != b) or a == b or (k == 3 and abs(a - b) <= 1e-9), (k, got, want)


def frozen_snapshot(env, e):
    out = {k: env.state.t[k][e].cpu().clone() for k in FROZEN}
    if env.gaze_state is not None and env.gaze_state.owl_state is not None:
        out['owl_state'] = env.gaze_state.owl_state[e].cpu().clone()
    return out


def same_frozen(a, b):
    import torch
    return all(torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)) for k in a)


def batch_of(pkg, backend, w=None, p=None, B=1, **kw):
    from drone2d_amd import runner
    p = params_of(pkg, w) if p is None else p
    return runner.SteppedExperimentBatch(p, B, device=str(getattr(backend, 'device', 'cpu')), backend=backend, jerk_tie=tie_table(), **kw)


def replay(pkg, backend, i):
    """world i, step for step through run_episodes(max_steps=1), then frozen; and in one run() of a fresh batch: the same row"""
    w = world(i)
    xb = batch_of(pkg, backend, w)
    env = xb.env
    T = len(w['t_done'])
    assert xb.params.gaze_method == w['cfg']['gaze_method'] and env.step_gaze == w['cfg']['gaze_method']
    for t in range(T):
        assert env.run_episodes(max_steps=1) == 1
        check_step(w, t, env)
    assert bool(env.state.flags[0, A.F_DONE])
    end = frozen_snapshot(env, 0)
    assert env.run_episodes(max_steps=3) == 3
    assert same_frozen(end, frozen_snapshot(env, 0))
    check_row(w, xb.rows()[0])
    whole = batch_of(pkg, backend, w)
    rows = whole.run(check_every=16)
    assert rows == xb.rows() or all((a != a and b != b) or a == b for a, b in zip(rows[0], xb.rows()[0]))
    assert T <= whole.steps_run <= min(whole.max_steps, (T + 15) // 16 * 16)
    assert same_frozen(end, frozen_snapshot(whole.env, 0))
    return xb


def staggered(pkg, backend, p, B=3):
    """a B-env batch whose envs end at different steps: each env's frozen fields stay bit-equal from its terminal step to the end of
    the run, and the rows equal B single-env runs"""
    xb = batch_of(pkg, backend, p=p, B=B)
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
        one = batch_of(pkg, backend, p=q, B=1)
        r = one.run()[0]
        assert one.steps_run >= ended[e] + 1
        assert all((a != a and b != b) or a == b for a, b in zip(r, rows[e])), (e, r, rows[e])
    return ended
