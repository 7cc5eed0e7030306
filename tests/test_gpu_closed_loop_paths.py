"""Every launch path of d2d_closed_loop against the oracle (run with -m gpu): the case table of closed_loop_cases.py -- the five
persistent kernels and the two per-stage loops, each with Oxford, LookAhead, LookGoal and a constant gaze, under CONTINUE, RESET
and FREEZE, with measurement noise rows, partial edge tiles and a NULL traj_box -- device vs oracle, every field of the env and
plugin state bit for bit after every call.  Every row asserts the path it was written for and shows that it ran what it is
there for (episodes ended, searches ran, trackers were active, LookGoal saw a trajectory).  Then the persistent kernel against
the forced per-stage loop at 257 envs."""
import numpy as np
import pytest
import torch

import closed_loop_cases as CL
from test_gpu_heading_gaze import _host_actions
from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import _worlds

pytestmark = pytest.mark.gpu

HEADING = ('LookAhead', 'LookGoal')
SCRATCH = ('nodes', 'hash', 'launch_args')      # plugin buffers whose contents mean nothing between calls


def _mode(c):
    return {'continue': {}, 'reset': dict(auto_reset=True), 'freeze': dict(freeze_done=True)}[c['on_done']]


def _envs(pkg, hip, oracle, c):
    """The row's device env and the oracle env on the same worlds.  The oracle's gaze stage knows only Oxford: under LookAhead /
    LookGoal it takes its actions from the package's host policy (gaze='external'), one step at a time."""
    from drone2d_amd import vec_env
    p, planner = CL.params_of(pkg, c), CL.planner_of(c)
    ref = vec_env.VecDrone2DEnv(p, c['B'], backend=oracle, planner=planner, device_plugins=True,
                                gaze='external' if c['gaze'] in HEADING else c['policy'])
    dev = vec_env.VecDrone2DEnv(p, c['B'], backend=hip, planner=planner, device_plugins=True, gaze=c['policy'],
                                worlds=_worlds(ref), grid_layout=c['layout'])
    CL.adjust_plan(c, dev._plan)
    if c['noise']:                                   # [T, B, N, 2]: a run wraps around the rows, and calls start mid-way
        noise = np.random.RandomState(c['kw']['map_id']).standard_normal((CL.NOISE_ROWS, c['B'], dev.N, 2))
        for env in (dev, ref):
            env.set_noise(noise)
    return dev, ref


def ref_step(pkg, ref, c, policy, seen):
    """One oracle step of row `c`; `seen` collects what the row has to show it exercised"""
    A = pkg._abi
    if policy is not None:
        done = ref.state.flags[:, A.F_DONE].numpy() != 0
        if c['on_done'] == 'reset' and done.any():        # the device resets a finished env at the start of its next step
            ref.reset(torch.from_numpy(done.astype(np.uint8)))
            done[:] = False
        envs = np.flatnonzero(~done) if c['on_done'] == 'freeze' else np.arange(ref.num_envs)   # a frozen env keeps its action
        hd = ref.plugins.t['traj_hdr'].numpy()
        seen['traj'] = seen['traj'] or bool((hd[envs, 1] > hd[envs, 0]).any())
        _host_actions(ref, policy, envs)
    ref.closed_loop(1, **_mode(c))
    seen['done'] = seen['done'] or bool(ref.state.flags[:, A.F_DONE].any())
    seen['active'] = max(seen['active'], int(ref.state.active.sum()))


def _check_boxes(dev, tag):
    """Every remaining waypoint lies inside the box of its 64-slot chunk (d2d_plan.traj_box): a box is a bound the walks trust"""
    hd, traj, box = (dev.plugins.t[k].cpu() for k in ('traj_hdr', 'traj', 'traj_box'))
    for e in range(dev.num_envs):
        h, n = int(hd[e, 0]), int(hd[e, 1])
        if n > h:
            xy, b = traj[e, h:n, :2], box[e, torch.arange(h, n) // 64]
            inside = (xy[:, 0] >= b[:, 0]) & (xy[:, 1] >= b[:, 1]) & (xy[:, 0] <= b[:, 2]) & (xy[:, 1] <= b[:, 3])
            bad = (~inside).nonzero().flatten()
            assert bad.numel() == 0, f'{tag}: env {e} waypoints {(bad[:5] + h).tolist()} outside their chunk box'


def _snapshot(env):
    env.sync()
    out = {'s.' + k: v.clone() for k, v in env.state.t.items()}
    out.update({'p.' + k: v.clone() for k, v in env.plugins.t.items()})
    return out, env.cfg.noise_row0


@pytest.mark.parametrize('case', CL.CASES, ids=CL.case_id)
def test_closed_loop_path_matches_oracle(pkg, hip, oracle, case):
    from drone2d_amd import gaze as G
    c, name = case, CL.case_id(case)
    dev, ref = _envs(pkg, hip, oracle, c)
    assert CL.closed_loop_path(dev.cfg, dev._plan) == c['path'], name
    policy = getattr(G, c['policy'])(ref.params) if c['gaze'] in HEADING else None
    primitive = CL.planner_of(c) == 'Primitive'
    seen = dict(done=False, active=0, traj=False)
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        t = 0
        for i, n in enumerate(CL.chunk_sizes(c)):
            if c['zero_call'] and i == 1:               # closed_loop(0) changes nothing, noise row included
                before, row0 = _snapshot(dev)
                dev.closed_loop(0, **_mode(c))
                after, row0_after = _snapshot(dev)
                assert row0 == row0_after and all(torch.equal(v, after[k]) for k, v in before.items()), name
            dev.closed_loop(n, **_mode(c))
            for _ in range(n):
                ref_step(pkg, ref, c, policy, seen)
            t += n
            _assert_same(dev, ref, f'{name} after step {t}')
            if primitive and not c['null_box']:
                _check_boxes(dev, f'{name} after step {t}')
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    # the row ran what it is there for
    assert seen['done'], f'{name}: no episode ended'
    if primitive:
        assert int(ref.plugins.t['plan_stat'][:, 0].sum()) > 0 and int(dev.plugins.t['plan_stat'][:, 0].sum()) > 0, name
    if c['noise']:
        assert seen['active'] > 0, f'{name}: no tracker was active'
    if c['gaze'] == 'LookGoal' and primitive:
        assert seen['traj'], f'{name}: LookGoal never saw a trajectory'
    if c['null_box']:
        assert not bool(dev.plugins.t['traj_box'].any()), name      # nothing wrote boxes the plan does not hand over


@pytest.mark.parametrize('policy', ['Oxford', 'LookGoal'])
def test_persistent_and_per_stage_paths_agree_at_257_envs(pkg, hip, policy):
    """A batch the oracle would be slow for, not a multiple of 4 and above 256: the persistent kernel and the forced per-stage
    loop (launch_args = NULL) on the same worlds, 60 steps with auto reset in uneven calls -- every env and plugin field
    bit-identical after every call."""
    from drone2d_amd import _abi as A, vec_env
    B = 257
    p = pkg.Params(planner='Primitive', gaze_method=policy, agent_number=12, map_id=400, **CL._NEAR, **CL._FAST)
    worlds = vec_env.build_worlds(p, B)
    envs = [vec_env.VecDrone2DEnv(p, B, backend=hip, planner='Primitive', device_plugins=True, gaze=policy, worlds=worlds)
            for _ in range(2)]
    envs[1]._plan.launch_args = None
    assert [CL.closed_loop_path(e.cfg, e._plan) for e in envs] == ['k_closed<1>', 'per_stage_primitive']
    t = 0
    for n in (1, 7, 16, 3, 13, 20):
        for e in envs:
            e.closed_loop(n, auto_reset=True)
        t += n
        a, b = (_snapshot(e)[0] for e in envs)
        for k in a:
            if k[2:] not in SCRATCH:
                assert torch.equal(a[k], b[k]), f'{policy}: {k} differs after step {t} at {(a[k] != b[k]).nonzero()[:5].tolist()}'
    assert t == 60 and bool((envs[0].state.counters[:, A.C_STEPS] < 60).any())          # episodes ended and restarted
    assert int(envs[0].plugins.t['plan_stat'][:, 0].min()) >= 1
    # give back the two batches' search scratch (2 x 0.5 GB): later tests would otherwise carve their buffers from these segments
    del envs, a, b
    torch.cuda.empty_cache()
