"""LookAhead / LookGoal as device gaze stages (run with -m gpu): the device atan2 against libm, the stage against the reference's
recorded values, traces, episodes and rows, and a randomised device-vs-oracle soak in which the oracle steps the package's host
policies (gaze='external': the oracle's own gaze stage knows only Oxford)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import replay
from replay import load
from test_atan2 import atan2_host, atan2_pairs, same_bits  # noqa: F401  (atan2_host: fixture)
from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import CFG5, _worlds
import host_build

pytestmark = pytest.mark.gpu


@host_build.needs_fma('libm dispatches a non-FMA atan2 variant on this CPU')
def test_device_atan2_is_bit_identical_to_libm(hip, atan2_host):
    y, x = atan2_pairs(seed=19)
    want = atan2_host[1](y, x)
    yd, xd = torch.from_numpy(y).to(hip.device), torch.from_numpy(x).to(hip.device)
    out = torch.empty_like(yd)
    hip.atan2_array(yd, xd, out)
    got = out.cpu().numpy()
    bad = np.flatnonzero(~same_bits(got, want))
    assert bad.size == 0, [(y[i].hex(), x[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:8]]


def test_gaze_stage_reproduces_reference_values(pkg, hip):
    """golden `host_gaze_values` (yaw_planner.LookAhead / LookGoal on 4000 random observations, drawn in the order of
    test_dropin_reference_plugins.py) injected into a 4000-env state: one d2d_gaze_stage per policy gives every value bit for bit."""
    from drone2d_amd import _abi as A, host_init, vec_env
    want, B = load('host_gaze_values')['values'], 4000
    rng = np.random.RandomState(11)
    drone, dmap = np.zeros((B, A.DF)), np.zeros((B, 50, 50), np.uint8)
    traj, hdr = None, np.zeros((B, 2), np.int32)
    pts_all = []
    for case in range(B):
        vel = rng.uniform(-40, 40, 2) * rng.choice([0, 1, 1, 1], 2)
        if case % 7 == 0:
            vel = np.round(vel)
        yaw = rng.uniform(-400, 800) if case % 3 else float(rng.randint(0, 360))
        x, y = float(rng.randint(0, 500)), float(rng.randint(0, 500))
        dmap[case] = rng.choice([0, 1, 2], (50, 50), p=[0.2, 0.1, 0.7]).astype(np.uint8)
        pts = [np.round(rng.uniform(-20, 520, 2)) for _ in range(rng.randint(0, 12))]
        if case % 11 == 0 and pts:
            pts[-1] = np.array([x, y])                                            # atan2(-0.0, 0.0)
        drone[case, [A.D_X, A.D_Y, A.D_YAW, A.D_VX, A.D_VY]] = [x, y, yaw, vel[0], vel[1]]
        pts_all.append(pts)
    for j, gaze in enumerate(('LookAhead', 'LookGoal')):
        p = pkg.Params(planner='Primitive', gaze_method=gaze, agent_number=2, agent_radius=10, map_id=1)
        w = host_init.init_world(pkg.with_defaults(p))
        env = vec_env.VecDrone2DEnv(p, B, backend=hip, planner='Primitive', device_plugins=True, gaze=gaze, worlds=[w] * B)
        assert (env.cfg.W, env.cfg.grid_tile, env._plan.gaze) == (50, 0, 2 + j)
        if traj is None:
            traj = np.zeros(tuple(env.plugins.t['traj'].shape))
            for e, pts in enumerate(pts_all):                  # the remaining waypoints need not start at slot 0
                hdr[e] = [e % 5, e % 5 + len(pts)]
                for k, q in enumerate(pts):
                    traj[e, e % 5 + k, :2] = q
        env.state.drone.copy_(torch.from_numpy(drone))
        env.state.dmap.copy_(torch.from_numpy(dmap))
        env.plugins.t['traj'].copy_(torch.from_numpy(traj))
        env.plugins.t['traj_hdr'].copy_(torch.from_numpy(hdr))
        hip.gaze_stage(env.cfg, env._st, env._plan)
        got = env.state.action.cpu().numpy()
        bad = np.flatnonzero(got.view(np.int64) != want[:, j].view(np.int64))
        assert bad.size == 0, (gaze, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8], j].tolist())


@pytest.mark.parametrize('name', ['lookahead_primitive_n30_map0', 'lookahead_primitive_n30_map3', 'deadlock_primitive'])
def test_lookahead_stage_replays_reference_traces(pkg, hip, name):
    """The recorded LookAhead + Primitive episodes replayed stage by stage (as test_plugins_cpu replays Oxford) with the device
    gaze stage computing the action: action, plan() result, head waypoint, trajectory length and the whole state every step."""
    from drone2d_amd import device_plugins as DP
    R = replay.Replay(pkg, hip, name, kf=True)
    ps = DP.PluginState(R.p, R.cfg, hip.device, R.world['tracker_radius'][None], planner='Primitive', gaze='LookAhead')
    plan, fx = ps.struct(), R.fx
    for t in range(R.T):
        s, tag = R.st.struct(), f'{name} step {t + 1}: '
        hip.gaze_stage(R.cfg, s, plan)
        assert float(R.st.action[0]) == float(fx['t_action'][t]), tag + 'gaze action'
        hip.perceive(R.cfg, s)
        hip.plan_stage(R.cfg, s, plan)
        assert int(R.st.plan_ok[0]) == int(fx['t_plan_ok'][t]), tag + 'plan() result'
        assert int(R.st.wp_valid[0]) == int(fx['t_wp_valid'][t]), tag + 'trajectory empty / not'
        if fx['t_wp_valid'][t]:
            assert np.array_equal(R.st.wp[0].cpu().numpy(), fx['t_wp'][t]), tag + 'head waypoint'
        hdr = ps.t['traj_hdr'][0].cpu().numpy()
        assert int(hdr[1] - hdr[0]) == int(fx['t_traj_len'][t]), tag + 'len(trajectory)'
        hip.act(R.cfg, s)
        hip.sync()
        R.compare(t)


def _row(r):
    return np.array([float(v) for v in r[12:]], dtype=np.float64)


def _batch(pkg, hip, fixture, case, B):
    from drone2d_amd import runner
    fx = load(fixture)
    kw = json.loads(str(fx[f'r{case}_cfg']))
    p = pkg.Params(debug=True, **kw)
    p.render = False
    eb = runner.ExperimentBatch(p, B, device=hip.device, backend=hip)
    assert not eb._host_lookahead and eb.env._plan.gaze == {'LookAhead': 2, 'LookGoal': 3}[kw['gaze_method']]
    return fx, kw, eb


@pytest.mark.parametrize('case', [0, 1, 2])
def test_reference_episodes_as_device_closed_loops(pkg, hip, case):
    """golden `host_gaze_rows` cases 0-1 (LookGoal) and 2 (LookAhead) as device closed loops, one step per call: every action
    and the CSV row equal the reference's."""
    fx, _, eb = _batch(pkg, hip, 'host_gaze_rows', case, 1)
    acts = []
    while not acts or not bool(eb.env.state.flags[0, pkg._abi.F_DONE]):
        eb.env.closed_loop(1, freeze_done=True)
        acts.append(float(eb.env.state.action[0]))
    acts, want = np.array(acts), fx[f'r{case}_actions']
    assert len(acts) == len(want) and np.array_equal(acts.view(np.int64), want.view(np.int64)), \
        f'case {case}: first difference at step {int(np.argmax(acts[:len(want)] != want[:len(acts)]))}'
    assert np.allclose(_row(eb.rows()[0]), fx[f'r{case}_row'], rtol=0, atol=1e-9, equal_nan=True)


@pytest.mark.parametrize('fixture,case', [('experiment_rows', 1), ('host_gaze_rows', 0)])
def test_experiment_batch_device_heading_gaze(pkg, hip, fixture, case):
    """ExperimentBatch with LookAhead (experiment_rows r1, main.py's default pair) and LookGoal as device stages: row 0 is the
    reference's row, rows >= 1 equal stand-alone Experiment runs (the package's host policy objects on the env facade)."""
    from drone2d_amd import runner
    fx, kw, eb = _batch(pkg, hip, fixture, case, 5)
    rows = eb.run()
    assert all(int(d) for d in eb.env.state.flags[:, pkg._abi.F_DONE].cpu())
    assert np.allclose(_row(rows[0]), fx[f'r{case}_row'], rtol=0, atol=1e-9, equal_nan=True), _row(rows[0])
    for e in range(1, 5):
        q = pkg.Params(debug=True, **dict(kw, map_id=kw['map_id'] + e))
        q.render = False
        want = runner.Experiment(q, device=hip.device, backend=hip).run()
        assert rows[e][3] == want[3] and np.allclose(_row(rows[e]), _row(want), rtol=0, atol=1e-9, equal_nan=True), e


class _Map:
    """drone.map.get_grid (utils.py:545-548) over the oracle's explored map"""

    def __init__(self, g, p):
        self.g, self.w, self.h, self.s = g, p.map_size[0], p.map_size[1], p.map_scale

    def get_grid(self, x, y):
        return 1 if (x >= self.w or x < 0 or y >= self.h or y < 0) else self.g[int(x // self.s), int(y // self.s)]


def _host_actions(env, policy, envs):
    """The package's host policy (gaze.LookAhead / LookGoal, equal to the reference's classes) on the oracle's state"""
    from drone2d_amd import _abi as A
    d, dm = env.state.drone.numpy(), env.state.logical('dmap').numpy()
    for e in envs:
        drone = types.SimpleNamespace(velocity=d[e, [A.D_VX, A.D_VY]], yaw=float(d[e, A.D_YAW]), x=float(d[e, A.D_X]),
                                      y=float(d[e, A.D_Y]), map=_Map(dm[e], env.params))
        traj = types.SimpleNamespace(positions=list(env.plugins.trajectory(e)[0]))
        env.state.action[e] = float(policy.plan({'drone': drone, 'trajectory': traj, 'target': None}))


def _soak_cfg(seed):
    rng = np.random.RandomState(5000 + seed)
    kw = dict(agent_number=int(rng.randint(2, 41)), agent_radius=int(rng.choice([5, 8, 10, 12, 15])),
              agent_max_speed=int(rng.choice([10, 20, 30, 40, 60])), drone_max_speed=int(rng.choice([20, 30, 40, 50])),
              map_id=int(rng.randint(0, 10000)), drone_view_range=int(rng.choice([60, 90, 120, 360])),
              drone_view_depth=int(rng.choice([60, 80, 100])), drone_max_yaw_speed=int(rng.choice([40, 80, 120])))
    if rng.rand() < 0.25:
        kw['static_map'] = str(rng.choice(['maps/obstacle_map.npy', 'maps/shaped_obstacle_map.npy']))
    if rng.rand() < 0.3:
        kw['target_list'] = [[int(rng.randint(40, 460)), int(rng.randint(40, 460))]]
    if rng.rand() < 0.25:
        kw['max_flight_time'] = 6
    return kw, dict(gaze=('LookAhead', 'LookGoal')[seed % 2], planner='NoMove' if seed % 9 == 4 else 'Primitive',
                    B=int(rng.choice([3, 4, 6])), chunk=int(rng.choice([1, 4, 8, 15])), auto=seed % 3 != 0)


@pytest.mark.parametrize('seed', list(range(int(os.environ.get('D2D_HEADING_SEEDS', '36')))) + ['config5'])
def test_random_heading_gaze_matches_oracle(pkg, hip, oracle, seed):
    """Device closed loop with LookAhead / LookGoal for 120 steps (auto reset or freeze) vs the oracle stepping the same batch one
    step at a time with the host policy's actions: the whole env and plugin state, actions included, bit for bit at every chunk.
    'config5': BASELINE config 5's 640 x 640-cell geometry on tiled device grids."""
    from drone2d_amd import gaze as G, vec_env
    if seed == 'config5':
        kw, r = dict(CFG5, agent_number=40, drone_max_speed=40, map_id=5), dict(gaze='LookGoal', planner='Primitive', B=2, chunk=8,
                                                                              auto=True)
    else:
        kw, r = _soak_cfg(seed)
    p = pkg.Params(planner=r['planner'], gaze_method=r['gaze'], **kw)
    ref = vec_env.VecDrone2DEnv(p, r['B'], backend=oracle, planner=r['planner'], device_plugins=True, gaze='external')
    dev = vec_env.VecDrone2DEnv(p, r['B'], backend=hip, planner=r['planner'], device_plugins=True, gaze=r['gaze'],
                                worlds=_worlds(ref))
    assert seed != 'config5' or dev.cfg.grid_tile == 16
    policy = getattr(G, r['gaze'])(ref.params)
    mode = dict(auto_reset=True) if r['auto'] else dict(freeze_done=True)
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        for t0 in range(0, 120, r['chunk']):
            n = min(r['chunk'], 120 - t0)
            dev.closed_loop(n, **mode)
            for _ in range(n):
                done = ref.state.flags[:, pkg._abi.F_DONE].numpy() != 0
                if r['auto'] and done.any():        # the device resets a finished env at the start of its next step
                    ref.reset(torch.from_numpy(done.astype(np.uint8)))
                    done[:] = False
                _host_actions(ref, policy, np.flatnonzero(~done))    # a frozen env keeps its last action
                ref.closed_loop(1, **mode)
            _assert_same(dev, ref, f'seed {seed} {r} {kw} after step {t0 + n}')
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
