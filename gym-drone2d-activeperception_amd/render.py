"""The renderer's Python side (include/d2d_render.h; VecDrone2DEnv.render_list / render_frames, Drone2DEnv2.render('rgb_array')): the
call struct of a set of slots, the scratch it points at, and the two launches.  Nothing here reads the device.

Lists and frames are scratch, never state: they hang on a RenderScratch object, which is no holder of fork.slot_tensors."""
import math

import numpy as np
import torch

from . import _abi as A
from ._lib import backend_for

STAR = [f(math.pi / 5 * i) for i in range(10) for f in (math.sin, math.cos)]      # utils.py:43-49, the host's libm


class RenderScratch:
    """The list buffers of the latest call, kept for the next one of the same size"""
    key = None
    items = bbox = count = status = None


def frame_shape(cfg, downsample):
    d = int(downsample)
    return -(-int(cfg.H_px) // d), -(-int(cfg.W_px) // d)


def slots_of(env, slots):
    """[S] int32 on the env's device; a list is checked here, a tensor's values by the launch (a slot outside the batch draws nothing)"""
    if slots is None:
        return torch.arange(env.num_envs, dtype=torch.int32, device=env.device)
    if not isinstance(slots, torch.Tensor):
        arr = np.asarray(slots, dtype=np.int64).reshape(-1)
        if arr.size and (arr.min() < 0 or arr.max() >= env.num_envs):
            raise IndexError(f'render: slots {arr.tolist()} of an env with {env.num_envs} slots')
        slots = torch.from_numpy(arr)
    if slots.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'render: slots is an int32 or int64 tensor or a list (got {slots.dtype})')
    return slots.reshape(-1).to(device=env.device, dtype=torch.int32).contiguous()


def _trajectories(env, trajectories, S):
    """(traj [S, K, 2] float64, traj_len [S] int32) on the device from a pair of such tensors, or from a list of S arrays [n_i, 2]"""
    if trajectories is None:
        return None, None
    if isinstance(trajectories, (tuple, list)) and len(trajectories) == 2 and isinstance(trajectories[0], torch.Tensor) \
            and trajectories[0].dim() == 3:
        traj, n = trajectories
    else:
        rows = [np.asarray(t, dtype=np.float64).reshape(-1, 2) for t in trajectories]
        K = max([len(r) for r in rows] + [1])
        pad = np.zeros((len(rows), K, 2))
        for i, r in enumerate(rows):
            pad[i, :len(r)] = r
        traj, n = torch.from_numpy(pad), torch.tensor([len(r) for r in rows], dtype=torch.int32)
    if traj.shape[0] != S or n.shape[0] != S or traj.shape[2] != 2:
        raise ValueError(f'render: trajectories for {traj.shape[0]} slots, {S} chosen')
    return (traj.to(device=env.device, dtype=torch.float64).contiguous(), n.to(device=env.device, dtype=torch.int32).contiguous())


def _ready(env, downsample):
    """the refusals that come before anything is allocated; returns the downsample as an int"""
    backend_for(env.backend, None, 'supports_render', 'has no renderer (include/d2d_render.h: render_list() / render_frames() run on the '
                'HIP backend, with csrc/render/libd2d_render.so built)')
    d = int(downsample)
    if d != downsample or not 1 <= d <= A.RENDER_MAX_DOWNSAMPLE:
        raise ValueError(f'render: downsample {downsample!r}: an integer 1 .. {A.RENDER_MAX_DOWNSAMPLE}')
    return d


def call_of(env, slots, downsample=1, trajectories=None, cap=None, scratch=None):
    """(_abi.RenderCall, the tensors it points at) for `slots` [S] int32.  `cap`: the list capacity in place of the one derived from
    P, N and the trajectory capacity (the tests make it too small by hand).  `scratch`: a RenderScratch of the caller's own in place
    of the env's (capture.Capture keeps one)"""
    d = _ready(env, downsample)
    s, S = env.state, int(slots.numel())
    traj, traj_len = _trajectories(env, trajectories, S)
    plan = env.plugins.t if env.plugins is not None and env.plugins.planner == A.PLAN_PRIMITIVE and traj is None else None
    pillars = s.t.get('pillars')            # (hand-built host worlds that name no obstacles keep none)
    P, N = int(pillars.shape[1]) if pillars is not None else 0, env.cfg.N
    K = int(traj.shape[1]) if traj is not None else 0
    plan_cap = int(plan['traj'].shape[1]) if plan is not None else 0
    cap = A.render_cap(P, N, max(K, plan_cap)) if cap is None else int(cap)
    sc = scratch if scratch is not None else env.__dict__.setdefault('_render', RenderScratch())
    if sc.key != (S, cap):
        dev = env.device
        sc.items = torch.zeros((S, cap, A.RENDER_ITEM_BYTES), dtype=torch.uint8, device=dev)
        sc.bbox = torch.zeros((S, cap, 4), dtype=torch.int16, device=dev)
        sc.count = torch.zeros(S, dtype=torch.int32, device=dev)
        sc.status = torch.zeros(S, dtype=torch.uint8, device=dev)
        sc.key = (S, cap)
    c = A.RenderCall()
    keep = dict(slots=slots, pillars=pillars if P else None, agent_vel=s.agent_vel if env.rvo and N else None,
                plan_traj=plan['traj'] if plan is not None else None, plan_hdr=plan['traj_hdr'] if plan is not None else None,
                traj=traj, traj_len=traj_len, items=sc.items, bbox=sc.bbox, count=sc.count, status=sc.status, frame=None)
    for n, t in keep.items():
        setattr(c, n, t.data_ptr() if t is not None and t.numel() else None)
    c.S, c.P, c.K, c.plan_cap, c.cap, c.downsample = S, P, K, plan_cap, cap, d
    c.n_seeded = min(int(env.params.agent_number), N)
    c.view_range = float(env.params.drone_view_range)
    c.star[:] = STAR
    return c, keep


def lists(env, slots=None, trajectories=None, cap=None):
    """VecDrone2DEnv.render_list"""
    _ready(env, 1)
    slots = slots_of(env, slots)
    c, keep = call_of(env, slots, 1, trajectories, cap)
    if c.S:
        env.backend.render_list(env.cfg, env._st, c)
    return views(keep['items'], keep['count'], keep['status'])


def views(items, count, status):
    """the fields of d2d_render_item as tensors over the packed records [S, cap, 176]"""
    return {'kind': items[..., 0:4].contiguous().view(torch.int32)[..., 0], 'rgb': items[..., 4:7], 'npts': items[..., 7],
            'width': items[..., 8:16].contiguous().view(torch.float64)[..., 0],
            'geom': items[..., 16:A.RENDER_ITEM_BYTES].contiguous().view(torch.float64), 'count': count, 'status': status}


def frames(env, slots=None, downsample=1, out=None, trajectories=None, cap=None):
    """VecDrone2DEnv.render_frames"""
    downsample = _ready(env, downsample)
    slots = slots_of(env, slots)
    S = int(slots.numel())
    Hf, Wf = frame_shape(env.cfg, downsample)
    if out is None:
        out = torch.empty((S, Hf, Wf, 3), dtype=torch.uint8, device=env.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == env.state.action.device and out.is_contiguous()
              and out.dim() == 4 and out.shape[0] >= S and tuple(out.shape[1:]) == (Hf, Wf, 3)):
        raise ValueError(f'render_frames(): out is a contiguous uint8 tensor [>= {S}, {Hf}, {Wf}, 3] on {env.device}')
    if S == 0:
        return out[:0]
    c, keep = call_of(env, slots, downsample, trajectories, cap)
    c.frame = out.data_ptr()
    env.backend.render_list(env.cfg, env._st, c)
    env.backend.render_frame(env.cfg, env._st, c)
    return out[:S]
