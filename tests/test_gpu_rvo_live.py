"""The two launches of include/d2d_rvo_live.h (libd2d_rvo.so) on the device, run with -m gpu: a live env gets bit for bit what
d2d_rvo_velocity / d2d_rvo_agents_step give it, a finished env's vel_out is its vel and its agents keep every byte.  Shapes: a small
batch with the middle env done, one partial block of the move kernel, a finished env whose agents straddle the move kernel's
256-thread block boundary, and one agent without pillars (no cone).  Each with its own pattern, all done and none done.  Outputs sit
inside poisoned buffers whose padding is compared afterwards."""
import numpy as np
import pytest
import torch

import rvo_cases as RC
import rvo_model as M
from test_gpu_rvo import in_poison, padding_intact

pytestmark = pytest.mark.gpu
# B, N, P, the envs that are done
SHAPES = [(3, 5, 2, (1,)), (7, 10, 0, (0, 6)), (40, 10, 3, (25,)), (5, 1, 0, (1, 3))]


def inputs(B, N, P, dev):
    scenes = [RC.scene(N, P, 500 + 31 * B + k, 'cluster' if k % 2 else 'spread') for k in range(B)]
    ag = torch.from_numpy(np.stack([M.planes(s['pos'], s['pref'], s['radius']) for s in scenes])).to(dev)
    vel = torch.from_numpy(np.stack([np.ascontiguousarray(s['vel'].T.reshape(2, N)) for s in scenes])).to(dev)
    pil = torch.from_numpy(np.stack([s['pillars'].reshape(P, 3) for s in scenes]).astype(np.int32)).to(dev)
    return ag, vel, pil


def bytes_equal(a, b):
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))   # (reshape: empty selections too)


@pytest.fixture(scope='module')
def unmasked(hip):
    """(inputs, what the unmasked launches make of them), once per shape"""
    out = {}
    for B, N, P, _ in SHAPES:
        ag, vel, pil = inputs(B, N, P, hip.device)
        moved, vel_out = ag.clone(), torch.full_like(vel, float('nan'))
        hip.rvo_velocity(ag, vel, pil, vel_out)
        hip.rvo_agents_step(moved, vel_out, 500.0, 500.0, 10.0, 0.1)
        hip.sync()
        assert bool(torch.isfinite(vel_out).all()) and not torch.equal(moved, ag)
        out[(B, N, P)] = (ag, vel, pil, vel_out, moved)
    return out


@pytest.mark.parametrize('pattern', ['some', 'all', 'none'])
@pytest.mark.parametrize('B,N,P,done', SHAPES, ids=[f'B{s[0]}_N{s[1]}_P{s[2]}' for s in SHAPES])
def test_live_envs_equal_the_unmasked_launches_and_finished_envs_keep_everything(hip, unmasked, B, N, P, done, pattern):
    dev = hip.device
    ag0, vel0, pil0, want_vel, want_ag = unmasked[(B, N, P)]
    fin = torch.zeros(B, dtype=torch.bool)
    fin[list({'some': done, 'all': range(B), 'none': ()}[pattern])] = True
    flags = torch.randint(0, 2, (B, 4), dtype=torch.uint8)           # the other three bytes decide nothing
    flags[:, 3] = fin.to(torch.uint8) * torch.tensor([1, 2, 255] * B)[:B].to(torch.uint8)     # any non-zero byte says done
    flags, fin = flags.to(dev), fin.to(dev)
    ag_buf, ag = in_poison((B, 6, N), dev)
    ag.copy_(ag0)
    vel, pil, flags0 = vel0.clone(), pil0.clone(), flags.clone()
    out_buf, out = in_poison((B, 2, N), dev)
    out.fill_(float('nan'))
    hip.rvo_velocity_live(ag, vel, pil, flags, out)
    hip.sync()
    assert bytes_equal(ag, ag0) and bytes_equal(vel, vel0) and torch.equal(pil, pil0) and torch.equal(flags, flags0)   # inputs intact
    assert padding_intact(out_buf, B * 2 * N) and padding_intact(ag_buf, B * 6 * N)
    assert not bool(torch.isnan(out).any())                                                   # every entry written
    assert bytes_equal(out[~fin], want_vel[~fin]) and bytes_equal(out[fin], vel0[fin])
    out0 = out.clone()
    hip.rvo_agents_step_live(ag, out, flags, 500.0, 500.0, 10.0, 0.1)
    hip.sync()
    assert bytes_equal(out, out0) and torch.equal(flags, flags0)
    assert padding_intact(out_buf, B * 2 * N) and padding_intact(ag_buf, B * 6 * N)
    assert bytes_equal(ag[~fin], want_ag[~fin]) and bytes_equal(ag[fin], ag0[fin])
    if pattern == 'some' and N > 1:
        assert not bytes_equal(want_ag[fin], ag0[fin]) and not bytes_equal(want_vel[fin], vel0[fin])   # the mask had something to keep
    if (B, N) == (40, 10):
        assert 25 * N < 256 < 26 * N                                  # env 25's agents lie on both sides of the block boundary


def test_flags_null_is_refused_and_nothing_is_launched(hip):
    from drone2d_amd import _lib
    B, N, P = 3, 5, 2
    ag, vel, pil = inputs(B, N, P, hip.device)
    ag0 = ag.clone()
    out = torch.full_like(vel, float('nan'))
    with pytest.raises(_lib.D2DError, match='error -1: d2d_rvo_velocity_live: flags is NULL'):
        hip.rvo_velocity_live(ag, vel, pil, None, out)
    with pytest.raises(_lib.D2DError, match='error -1: d2d_rvo_agents_step_live: flags is NULL'):
        hip.rvo_agents_step_live(ag, vel, None, 500.0, 500.0, 10.0, 0.1)
    flags = torch.zeros((B, 4), dtype=torch.uint8, device=hip.device)
    with pytest.raises(_lib.D2DError, match='vel_out must not be vel'):
        hip.rvo_velocity_live(ag, vel, pil, flags, vel)
    hip.sync()
    assert bool(torch.isnan(out).all()) and bytes_equal(ag, ag0)
