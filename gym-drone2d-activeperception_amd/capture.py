"""Capture — the terminal frames of streamed episodes, chosen and drawn on the device (include/d2d_capture.h).

A stream rebuilds a finished slot in place at its next turn, and what survives of the episode is its record of eight numbers.  A
Capture handed to the stream (VecDrone2DEnv.stream_episodes(capture=), stream_rounds(capture=), action_stream(capture=),
runner.EpisodeStream with params.record_img) queues three launches in front of every d2d_stream_harvest: d2d_capture_select picks, among
the slots the harvest is about to record, those whose episode ended in one of `kinds`; d2d_render_list_sel and d2d_render_frame_sel
draw them into the next free frames of a gallery.  They are queued unconditionally and nothing is read back: `taken()` is the one
host read, for the caller to make when it wants the pictures.

    cap = Capture(env, kinds=('static', 'dynamic'), capacity=256, downsample=1, per_turn=64)
    rows = env.stream_episodes(100_000, capture=cap)
    n = cap.taken()
    cap.frames[:n], cap.meta[:n], cap.pose[:n]      # [n, Hf, Wf, 3] uint8, [n, 4] int32 (episode, kind, steps, slot), [n, 3] float64
    cap.save(img_dir)                               # <prefix>_<kind name>_<episode>.png

ORDER AND OVERFLOW.  The gallery is in arrival order: by turn, and by slot inside a turn.  Which slot plays an episode and the turn
that finds it finished follow from the refill schedule (`refill_every`, the number of slots), so the order does too -- sort by
meta[:, 0], the episode number.  At most `per_turn` slots are drawn per turn and `capacity` in all; the matches beyond either are
counted in dropped() and gone, and WHICH episodes those are depends on the schedule as well.  taken() + dropped() == matched() always.
A frame itself depends on nothing but its episode.

The reference saves a screenshot when the drone collides (params.record_img, envs/training_v3.py:180-187: '<gaze>_static_...' and
'<gaze>_dynamic_...', only when gaze_method != 'NoControl').  It saves self.screen, which holds the picture of the previous render()
call; this saves the terminal state's own picture.  The episode number stands where the reference writes datetime.now(), so that a
rerun writes the same files.  Not drawn: anything from before the terminal step (a slot has no history), text and covariance ellipses
(as in the renderer).  closed_loop(auto_reset=True) restarts envs inside a launch and has no moment to capture at.

All buffers hang on the Capture object: none is a per-slot tensor of a holder that fork.slot_tensors walks, and the list scratch is
the capture's own, not the env's."""
import os
import struct
import zlib

import numpy as np
import torch

from . import _abi as A
from . import render
from ._lib import backend_for

ALL_KINDS = A.CAPTURE_KIND_NAMES
EPISODE_DIGITS = 9               # STREAM_MAX_EPISODES has nine
DEFAULT_PER_TURN = 64


def kind_mask(kinds):
    """bit (k - 1) for every kind name of `kinds` (D2D_CAPTURE_*)"""
    if isinstance(kinds, str):
        kinds = (kinds,)
    mask = 0
    for name in kinds:
        if name not in ALL_KINDS:
            raise ValueError(f'Capture: kind {name!r}: one of {", ".join(ALL_KINDS)}')
        mask |= 1 << ALL_KINDS.index(name)
    return mask


def png_bytes(rgb):
    """The PNG file of an [H, W, 3] uint8 array: 8-bit RGB, one IDAT, every row with filter 0"""
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'png_bytes: an [H, W, 3] uint8 array (got {a.shape})')
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)         # column 0: the filter byte
    raw[:, 1:] = a.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + chunk(b'IEND', b''))


def file_name(prefix, kind, episode):
    """'<prefix>_<kind name>_<episode, zero-padded>.png' (envs/training_v3.py:181,185 with the episode in place of the clock)"""
    return f'{prefix}_{ALL_KINDS[int(kind) - 1]}_{int(episode):0{EPISODE_DIGITS}d}.png'


class Capture:
    """See the module's text.  `kinds`: names out of ALL_KINDS ('static', 'dynamic', 'dead_lock', 'freezing', 'goal', 'other': how
    the episode ended, the first that holds); `capacity`: frames of the gallery; `downsample`: render_frames()'s; `per_turn`: the
    slots drawn per turn at most, 1 .. num_envs (the list scratch is sized by it; default min(64, num_envs))."""

    def __init__(self, env, kinds=('static', 'dynamic'), capacity=256, downsample=1, per_turn=None):
        backend_for(env.backend, None, 'supports_capture', 'has no capture (include/d2d_capture.h: it runs on the HIP backend, with a '
                    'csrc/render/libd2d_render.so that has d2d_capture_select, d2d_render_list_sel and d2d_render_frame_sel)')
        self.downsample = render._ready(env, downsample)           # the renderer's own refusals
        self.kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        self.kind_mask = kind_mask(self.kinds)
        if int(capacity) != capacity or capacity < 1:
            raise ValueError(f'Capture: capacity {capacity!r}: an integer >= 1')
        if per_turn is None:
            per_turn = min(DEFAULT_PER_TURN, env.num_envs)
        if int(per_turn) != per_turn or not 1 <= per_turn <= env.num_envs:
            raise ValueError(f'Capture: per_turn {per_turn!r}: an integer 1 .. num_envs = {env.num_envs}')
        self.env, self.capacity, self.per_turn = env, int(capacity), int(per_turn)
        dev = env.device
        Hf, Wf = render.frame_shape(env.cfg, self.downsample)
        self.frames = torch.zeros((self.capacity, Hf, Wf, 3), dtype=torch.uint8, device=dev)
        self.meta = torch.full((self.capacity, A.CAPTURE_META_F), -1, dtype=torch.int32, device=dev)
        self.pose = torch.zeros((self.capacity, 3), dtype=torch.float64, device=dev)
        self.counts = torch.zeros(A.CAPTURE_COUNTS, dtype=torch.int64, device=dev)       # taken, dropped, matched
        self._turn = self._buffers(self.per_turn)
        self._owner = None

    # ------------------------------------------------------------------ the launches
    def _buffers(self, S):
        """(sel_slot, sel_dst, the list scratch, the calls made over them) for S entries a call"""
        dev = self.env.device
        return (torch.full((S,), -1, dtype=torch.int32, device=dev), torch.full((S,), -1, dtype=torch.int32, device=dev),
                render.RenderScratch(), {})

    def _call(self, buf):
        """the _abi.RenderCall over `buf`: its slots are the selection, its frames the gallery.  A call is kept only while every
        pointer in it is still the one render.call_of would write now -- under RVO the two halves of the velocity swap change places
        every step, and a tensor that was allocated anew (none is today: the env writes its state in place) makes a new call, never
        a read of freed memory.  The kept tensors outlive the launches"""
        sel_slot, _, scratch, calls = buf
        env, s = self.env, self.env.state
        plan = env.plugins.t if env.plugins is not None else {}
        key = tuple(t.data_ptr() if t is not None else 0 for t in (
            s.agent_vel if env.rvo and env.cfg.N else None, s.t.get('pillars'), plan.get('traj'), plan.get('traj_hdr'), self.frames))
        if key not in calls:
            c, keep = render.call_of(env, sel_slot, self.downsample, scratch=scratch)
            c.frame = self.frames.data_ptr()
            if len(calls) >= 4:                # (two under RVO, one otherwise, unless something was reallocated)
                calls.clear()
            calls[key] = (c, keep, self.frames)
        return calls[key][0]

    def queue(self, slot_episode=None, buf=None):
        """The three launches, now: select among the done slots (`slot_episode` [B] int32: those with an episode >= 0; None: all,
        episode = slot), then the lists and the frames of the chosen.  No host read"""
        env, b = self.env, self.env.backend
        buf = self._turn if buf is None else buf
        b.capture_select(env.cfg, env._st, slot_episode, self.kind_mask, buf[0], buf[1], self.meta, self.pose, self.counts)
        c = self._call(buf)
        b.render_list_sel(env.cfg, env._st, c)
        b.render_frame_sel(env.cfg, env._st, c, buf[1], self.capacity)

    def snapshot(self):
        """A batch env after run_episodes() (no stream: a finished env stays as it ended): every done slot of the capture's kinds goes
        into the gallery, episode = slot, in slot order -- all of them in one call whatever `per_turn` says, through a scratch of
        num_envs entries that is let go afterwards.  A second call takes them again"""
        if self._owner is not None:
            raise RuntimeError('Capture.snapshot(): the capture belongs to an open stream, whose turns fill it')
        if self.env.num_envs:
            self.queue(None, self._buffers(self.env.num_envs))
            self.env.sync()                # (the scratch outlives its launches)
        return self

    # ------------------------------------------------------------------ one stream at a time
    def check_free(self, env, owner=None):
        """the refusals of attach(), without taking the capture"""
        if env is not self.env:
            raise ValueError('capture=: the Capture was made for another env')
        if self._owner is not None and self._owner is not owner:
            raise RuntimeError('capture=: the Capture is in use by a stream that is still open (close() it, or let stream_episodes() '
                               'return); one gallery has one arrival order')

    def attach(self, env, owner):
        self.check_free(env, owner)
        self._owner = owner

    def detach(self, owner):
        if self._owner is owner:
            self._owner = None

    # ------------------------------------------------------------------ the host's side
    def taken(self):
        """frames in the gallery: a host read (a synchronisation)"""
        return int(self.counts[0])

    def dropped(self):
        """matches that found no room, in `per_turn` or in `capacity`"""
        return int(self.counts[1])

    def matched(self):
        return int(self.counts[2])

    def save(self, img_dir=None, prefix=None):
        """Writes the gallery as PNG files '<prefix>_<kind name>_<episode>.png' into `img_dir` (default: params.img_dir; made if
        missing) and returns their paths in gallery order.  `prefix` defaults to the env's gaze_method, as the reference's names start"""
        p = self.env.params
        img_dir = p.img_dir if img_dir is None else img_dir
        prefix = p.gaze_method if prefix is None else prefix
        n = self.taken()
        frames, meta = self.frames[:n].cpu().numpy(), self.meta[:n].cpu().numpy()
        if n:
            os.makedirs(img_dir or '.', exist_ok=True)
        paths = []
        for i in range(n):
            path = os.path.join(img_dir, file_name(prefix, meta[i, A.CAPTURE_M_KIND], meta[i, A.CAPTURE_M_EPISODE]))
            with open(path, 'wb') as f:
                f.write(png_bytes(frames[i]))
            paths.append(path)
        return paths
