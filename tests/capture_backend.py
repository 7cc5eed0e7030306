"""Test-side backends for capture.Capture without a GPU: the three launches of include/d2d_capture.h done on the host memory behind
their pointers -- the selection by tests/capture_model.py, the two skipping launches by tests/render_model.py as tests/render_backend.py
does the plain ones -- mixed into the stream backends of the other test modules, so that stream_episodes(capture=),
action_stream(capture=) and runner.EpisodeStream with record_img run on the host.  Test infrastructure: the product never imports this."""
import numpy as np

import capture_model as CM
import render_backend as RB
import render_cases as RC
import render_model as RM
import stream_model as SM
import tracks_backend as TB
from drone2d_amd import _abi as A
from drone2d_amd.state import untile_grid


class _Capture(RB._Render):
    supports_capture = True
    capture_launches = 0

    def capture_select(self, cfg, st, slot_episode, kinds, sel_slot, sel_dst, meta, pose, counts):
        B = cfg.B
        flags, counters = SM.at(st.flags, (B, 4), np.uint8), SM.at(st.counters, (B, A.CF), np.int32)
        drone = SM.at(st.drone, (B, A.DF), np.float64)
        self.capture_launches += 1
        CM.select(flags, counters, drone, None if slot_episode is None else slot_episode.numpy(), int(kinds), sel_slot.shape[0],
                  meta.shape[0], sel_slot.numpy(), sel_dst.numpy(), meta.numpy(), pose.numpy(), counts.numpy())

    def render_list_sel(self, cfg, st, c):
        slots = SM.at(c.slots, (c.S,), np.int32)
        skipped = slots == -1
        count, status = SM.at(c.count, (c.S,), np.int32), SM.at(c.status, (c.S,), np.uint8)
        self.render_list(cfg, st, c)
        count[skipped] = 0
        status[skipped] = A.RENDER_SKIPPED

    def render_frame_sel(self, cfg, st, c, dst, capacity):
        import torch
        B, S, cap, d = cfg.B, c.S, c.cap, c.downsample
        W_px, H_px, scale = int(cfg.W_px), int(cfg.H_px), int(cfg.scale)
        Hf, Wf = -(-H_px // d), -(-W_px // d)
        slots, items = SM.at(c.slots, (S,), np.int32), SM.at(c.items, (S, cap, RC.ITEM_BYTES), np.uint8)
        count, frame = SM.at(c.count, (S,), np.int32), SM.at(c.frame, (capacity, Hf, Wf, 3), np.uint8)
        gb = (-(-cfg.W // 16)) * (-(-cfg.H // 16)) * 256 if cfg.grid_tile else cfg.W * cfg.H
        grids = SM.at(st.dmap, (B, gb), np.uint8)
        for k, (e, to) in enumerate(zip(slots.tolist(), dst.numpy().tolist())):
            if e == -1 or not 0 <= to < capacity:
                continue
            if not 0 <= e < B:
                frame[to] = 240
                continue
            g = grids[e]
            cells = untile_grid(torch.from_numpy(g.copy())[None], cfg.W, cfg.H, cfg.grid_tile)[0].numpy() if cfg.grid_tile else g.reshape(cfg.W, cfg.H)
            frame[to] = RM.raster(RB.from_bytes(items[k], int(count[k])), cells, W_px, H_px, scale, d)


class CaptureTurnBackend(_Capture, TB.TracksTurnBackend):
    name = TB.TracksTurnBackend.name + '+render+capture'


class CaptureTurnJerkBackend(_Capture, TB.TracksTurnJerkBackend):
    name = TB.TracksTurnJerkBackend.name + '+render+capture'


def backend_for(params):
    return (CaptureTurnJerkBackend if params.planner == 'Jerk_Primitive' else CaptureTurnBackend)().of(params)


def env_of(params, slots, **kw):
    """VecDrone2DEnv of `params` with device worlds and the caller's gaze on a fresh backend that streams, renders and captures"""
    import action_stream_backend as AB
    return AB.env_of(params, slots, backend=backend_for(params), **kw)
