"""The two kernels of libd2d_rvo.so (include/d2d_rvo.h) against the Python model (tests/rvo_model.py), bit for bit: the synthetic
scenes the host build is held to in test_rvo_host_build.py, and the shapes at which the wave changes its path -- N = 63, 64, 65, 130
(one and more passes of 64 cone lanes), 161 and 193 candidates in one batch (the fourth candidate pass holds one lane), B = 1, 3, 67.
Outputs sit in the middle of poisoned buffers whose padding is compared afterwards; the inputs are compared with their copies."""
import numpy as np
import pytest
import torch

import rvo_cases as RC
import rvo_model as M

pytestmark = pytest.mark.gpu
POISON = -1.2345e300
PAD = 4096


def in_poison(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), POISON, dtype=torch.float64, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def padding_intact(buf, n):
    return bool((buf[:PAD] == POISON).all()) and bool((buf[PAD + n:] == POISON).all())


def run(hip, scenes):
    """scenes of one (N, P) as one batch through both launches -> (vel_out [B, N, 2], pos, pref) as numpy"""
    dev = hip.device
    B, N, P = len(scenes), len(scenes[0]['pos']), len(scenes[0]['pillars'])
    ag_buf, ag = in_poison((B, 6, N), dev)
    ag.copy_(torch.from_numpy(np.stack([M.planes(s['pos'], s['pref'], s['radius']) for s in scenes])))
    vel = torch.from_numpy(np.stack([np.ascontiguousarray(s['vel'].T.reshape(2, N)) for s in scenes])).to(dev)
    pil = torch.from_numpy(np.stack([s['pillars'].reshape(P, 3) for s in scenes]).astype(np.int32)).to(dev)
    out_buf, out = in_poison((B, 2, N), dev)
    ag0, vel0, pil0 = ag.clone(), vel.clone(), pil.clone()
    hip.rvo_velocity(ag, vel, pil, out)
    hip.sync()
    assert torch.equal(vel, vel0) and torch.equal(ag, ag0) and torch.equal(pil, pil0)          # the decision modifies no input
    assert padding_intact(out_buf, B * 2 * N) and padding_intact(ag_buf, B * 6 * N)
    assert N == 0 or not bool((out == POISON).any())                                          # every entry written
    got_vel = out.cpu().numpy().transpose(0, 2, 1).copy()
    out0 = out.clone()
    hip.rvo_agents_step(ag, out, 500.0, 500.0, 10.0, 0.1)
    hip.sync()
    assert torch.equal(out, out0) and torch.equal(ag[:, 4:], ag0[:, 4:])                       # rows R, R2 untouched
    assert padding_intact(out_buf, B * 2 * N) and padding_intact(ag_buf, B * 6 * N)
    a = ag.cpu().numpy()
    return got_vel, a[:, 0:2].transpose(0, 2, 1).copy(), a[:, 2:4].transpose(0, 2, 1).copy()


@pytest.mark.parametrize('N,P,kind', RC.SCENES)
def test_both_launches_equal_the_model_on_the_synthetic_scenes(hip, N, P, kind):
    s, mvel, mpos, mpref, ev = RC.scene_model(N, P, 100 + N + P, kind)
    vel, pos, pref = run(hip, [s])
    assert M.bits_equal(vel[0], mvel) and M.bits_equal(pos[0], mpos) and M.bits_equal(pref[0], mpref)
    assert ev.get(('C', 193), 0) >= 1 and (N == 1 or ev.get(('C', 161), 0) >= 1)               # 161 and 193 candidates in one batch


def sampled_model(s, agents):
    """the model's decision and move of the sampled agents only (a decision costs (N - 1 + P) * 161 atan2 in Python)"""
    rob = float(s['radius'][0]) + 0.01
    out = {}
    for i in agents:
        vx, vy = M.decide(i, s['pos'], s['vel'], s['pref'], rob, s['pillars'])[:2]
        px, py, fx, fy, _, _ = M.agent_step(float(s['pos'][i][0]), float(s['pos'][i][1]), vx, vy, float(s['pref'][i][0]),
                                            float(s['pref'][i][1]), float(s['radius'][i]), 500, 500, 10, 0.1)
        out[i] = ((vx, vy), (px, py), (fx, fy))
    return out


@pytest.mark.parametrize('N,P,kind', [(63, 1, 'cluster'), (63, 2, 'spread'), (130, 0, 'spread'), (130, 5, 'cluster')])
def test_cone_lane_boundaries(hip, N, P, kind):
    """N - 1 + P = 63, 64 (one pass of cone lanes, full and not), 129 and 134 (three passes); the scenes of 64 and 65 agents above
    give 63 .. 69.  The agents around the lane boundaries and a seeded sample are held to the model."""
    s = RC.scene(N, P, 7 * N + P, kind)
    vel, pos, pref = run(hip, [s])
    pick = sorted({0, 1, 2, 62, 63, 64, 65, N - 2, N - 1} & set(range(N)) | set(np.random.RandomState(N).choice(N, 6, replace=False).tolist()))
    for i, (v, p, f) in sampled_model(s, pick).items():
        assert M.bits_equal(vel[0, i], v) and M.bits_equal(pos[0, i], p) and M.bits_equal(pref[0, i], f), i
    # the agents outside the sample: finite, and either the preferred velocity or a grid candidate no faster than it
    speed = np.hypot(vel[0, :, 0], vel[0, :, 1])
    assert np.isfinite(vel).all() and (speed <= np.hypot(s['pref'][:, 0], s['pref'][:, 1]) + 0.03).all()


def test_the_largest_cone_count_the_wave_holds(hip):
    """N - 1 + P = D2D_RVO_MAX_CONES = 1024: 48 KB of dynamic LDS per wave, sixteen passes of cone lanes.  1000 agents and 25 pillars;
    the first, the last and three seeded agents are held to the model (a decision costs 1024 * 161 atan2 in Python)."""
    from drone2d_amd import _abi as A
    N, P = 1000, 25
    assert N - 1 + P == A.RVO_MAX_CONES
    s = RC.scene(N, P, 4242, 'spread')
    vel, pos, pref = run(hip, [s])
    for i, (v, p, f) in sampled_model(s, [0, 2, 511, 998, 999]).items():
        assert M.bits_equal(vel[0, i], v) and M.bits_equal(pos[0, i], p) and M.bits_equal(pref[0, i], f), i
    assert np.isfinite(vel).all()


@pytest.mark.parametrize('B', [1, 3, 67])
def test_batches(hip, B):
    """B envs of 4 agents and 2 pillars, each its own scene (clustered and spread alternate), all held to the model"""
    scenes = [RC.scene(4, 2, 1000 + k, 'cluster' if k % 2 else 'spread') for k in range(B)]
    vel, pos, pref = run(hip, scenes)
    kinds = set()
    for k, s in enumerate(scenes):
        ev = {}
        mpos, mvel, mpref = M.step_world(s['pos'], s['vel'], s['pref'], s['radius'], s['pillars'], events=ev)
        assert M.bits_equal(vel[k], mvel) and M.bits_equal(pos[k], mpos) and M.bits_equal(pref[k], mpref), k
        kinds |= {key for key in ev if isinstance(key, tuple)}
    if B == 67:
        assert {('kind', M.PREF), ('kind', M.GRID), ('kind', M.NO_SUITABLE), ('C', 161), ('C', 193)} <= kinds


def test_sizes_the_wave_cannot_hold_are_refused_and_no_agents_launch_nothing(hip):
    from drone2d_amd import _abi as A
    from drone2d_amd import _lib
    D2DError = _lib.D2DError
    dev = hip.device
    N = A.RVO_MAX_CONES + 2
    z = torch.zeros((1, 6, N), dtype=torch.float64, device=dev)
    v, out = torch.zeros((1, 2, N), dtype=torch.float64, device=dev), torch.full((1, 2, N), POISON, dtype=torch.float64, device=dev)
    with pytest.raises(D2DError, match='cones'):
        hip.rvo_velocity(z, v, torch.zeros((1, 0, 3), dtype=torch.int32, device=dev), out)
    with pytest.raises(D2DError, match='vel_out'):
        hip.rvo_velocity(z[:, :, :4].contiguous(), v, torch.zeros((1, 0, 3), dtype=torch.int32, device=dev), v)
    hip.sync()
    assert bool((out == POISON).all())
    e = torch.zeros((2, 6, 0), dtype=torch.float64, device=dev)
    hip.rvo_velocity(e, torch.zeros((2, 2, 0), dtype=torch.float64, device=dev), torch.zeros((2, 3, 3), dtype=torch.int32, device=dev),
                     torch.zeros((2, 2, 0), dtype=torch.float64, device=dev))
    hip.rvo_agents_step(e, torch.zeros((2, 2, 0), dtype=torch.float64, device=dev), 500, 500, 10, 0.1)
    hip.sync()
