"""Test-side backend for render_list() / render_frames() without a GPU: the launches of include/d2d_render.h done by
tests/render_model.py on the host memory behind the structs' pointers, mixed into the oracle backends of the other test modules.  The
CPU stand-in the other libraries' *_backend.py files are: it lets the Python surface (drone2d_amd/render.py, the facade) run on the
host.  It does not fill the item boxes, which are the device rasteriser's own.  Test infrastructure: the product never imports this."""
import numpy as np

import render_cases as RC
import render_model as RM
import stream_model as SM
import tracks_backend as TB
from drone2d_amd import _abi as A
from drone2d_amd.state import untile_grid


def from_bytes(raw, n):
    """the first n packed records [., 176] uint8 as the arrays of a list"""
    raw = np.ascontiguousarray(raw[:n])
    return dict(kind=raw[:, 0:4].copy().view(np.int32).reshape(n), rgb=raw[:, 4:7].copy(), npts=raw[:, 7].copy(),
                width=raw[:, 8:16].copy().view(np.float64).reshape(n), geom=raw[:, 16:].copy().view(np.float64).reshape(n, 20), count=n)


class _Render:
    supports_render = True
    render_launches = 0

    def render_list(self, cfg, st, c):
        B, N, S, cap = cfg.B, cfg.N, c.S, c.cap
        slots, items = SM.at(c.slots, (S,), np.int32), SM.at(c.items, (S, cap, RC.ITEM_BYTES), np.uint8)
        count, status = SM.at(c.count, (S,), np.int32), SM.at(c.status, (S,), np.uint8)
        drone, agents = SM.at(st.drone, (B, A.DF), np.float64), SM.at(st.agents, (B, A.AF, N), np.float64)
        active, target = SM.at(st.active, (B, N), np.uint8), SM.at(st.target, (B, 2), np.float64)
        counters, pillars = SM.at(st.counters, (B, A.CF), np.int32), SM.at(c.pillars, (B, c.P, 3), np.int32)
        vel = SM.at(c.agent_vel, (B, 2, N), np.float64) if c.agent_vel else None
        self.render_launches += 1
        for k, e in enumerate(slots.tolist()):
            if not 0 <= e < B:
                count[k], status[k] = 0, 2
                continue
            traj = None
            if c.traj:
                n = min(max(int(SM.at(c.traj_len, (S,), np.int32)[k]), 0), c.K)
                traj = SM.at(c.traj, (S, c.K, 2), np.float64)[k, :n]
            elif c.plan_traj:
                head, stored = SM.at(c.plan_hdr, (B, 2), np.int32)[e].tolist()
                traj = SM.at(c.plan_traj, (B, c.plan_cap, 4), np.float64)[e, head:stored, :2]
            lst = RM.make_list(drone[e], agents[e], active[e], None if vel is None else vel[e], target[e], pillars[e], traj, cfg.depth,
                               c.view_range, cfg.drone_radius, int(counters[e, A.C_STEPS]), c.n_seeded)
            n = int(lst['count'])
            if n > cap:
                count[k], status[k] = 0, A.RENDER_OVERFLOW
            else:
                items[k, :n] = RC.to_bytes(lst, n)
                count[k], status[k] = n, A.RENDER_OK

    def render_frame(self, cfg, st, c):
        import torch
        B, S, cap, d = cfg.B, c.S, c.cap, c.downsample
        W_px, H_px, scale = int(cfg.W_px), int(cfg.H_px), int(cfg.scale)
        Hf, Wf = -(-H_px // d), -(-W_px // d)
        slots, items = SM.at(c.slots, (S,), np.int32), SM.at(c.items, (S, cap, RC.ITEM_BYTES), np.uint8)
        count, frame = SM.at(c.count, (S,), np.int32), SM.at(c.frame, (S, Hf, Wf, 3), np.uint8)
        gb = (-(-cfg.W // 16)) * (-(-cfg.H // 16)) * 256 if cfg.grid_tile else cfg.W * cfg.H
        grids = SM.at(st.dmap, (B, gb), np.uint8)
        self.render_launches += 1
        for k, e in enumerate(slots.tolist()):
            if not 0 <= e < B:
                frame[k] = 240
                continue
            g = grids[e]
            cells = untile_grid(torch.from_numpy(g.copy())[None], cfg.W, cfg.H, cfg.grid_tile)[0].numpy() if cfg.grid_tile else g.reshape(cfg.W, cfg.H)
            frame[k] = RM.raster(from_bytes(items[k], int(count[k])), cells, W_px, H_px, scale, d)

    def render_raster(self, r):
        d = r.downsample
        Hf, Wf = -(-r.H_px // d), -(-r.W_px // d)
        items, count = SM.at(r.items, (r.S, r.cap, RC.ITEM_BYTES), np.uint8), SM.at(r.count, (r.S,), np.int32)
        cells, frame = SM.at(r.cells, (r.S, r.W, r.H), np.uint8), SM.at(r.frame, (r.S, Hf, Wf, 3), np.uint8)
        for k in range(r.S):
            frame[k] = RM.raster(from_bytes(items[k], int(count[k])), cells[k], r.W_px, r.H_px, r.scale, d)


class RenderOracleBackend(_Render, TB.TracksOracleBackend):
    name = TB.TracksOracleBackend.name + '+render'


class RenderJerkBackend(_Render, TB.TracksJerkBackend):
    name = TB.TracksJerkBackend.name + '+render'


def env_of(params, B, **kw):
    """VecDrone2DEnv of `params` with the caller's gaze on a fresh backend that renders by the model"""
    return TB.env_of(params, B, backend=(RenderJerkBackend if params.planner == 'Jerk_Primitive' else RenderOracleBackend)(), **kw)
