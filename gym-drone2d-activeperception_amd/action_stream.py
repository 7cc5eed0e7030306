"""ActionStream — a stream of seeded episodes over resident slots that the CALLER steps, one gaze action per slot and step
(VecDrone2DEnv.action_stream): the learner's surface, where runner.EpisodeStream is the experimenter's.

The upstream project learns the gaze action with PPO on gym-2d-perception-v2 (script/train.py, model/extractor.py).  Such a caller
holds B slots, hands in an action tensor and takes observation tensors out at every step, and wants a slot whose episode has ended
to be in a fresh seeded world at its next step without the host in the loop.  `step(actions)` is

  the turn   (every `refill_every` steps, at the START of the call, so that a slot's terminal observation, flags, counters and episode
             number stay readable, without a copy, until the caller steps again): d2d_stream_harvest, d2d_stream_assign or
             d2d_stream_assign_table, d2d_worlds_build_masked, d2d_stream_restore (include/d2d_worlds_turn.h: one launch for all that
             VecDrone2DEnv._refill_rest does with masked fills and d2d_stream_clear) and the masked resets -- all queued
             unconditionally, nothing read back.  With a capture.Capture the three launches of include/d2d_capture.h go in front of
             the harvest, here and in close(), queued as unconditionally
  actions    written for the slots that play; a slot that is done or retired keeps its action, as it keeps everything else
  one step   of the env's own episode loop with every launch leaving finished slots alone (VecDrone2DEnv._episode_steps)
  explored   d2d_stream_explored: every slot's count of discovered cells, and its increase over the previous step

and no host read.  The reference's reward is 0 (drone_v2.py:257) and the ported `reward` stays 0: `terms` are what a reward is made of.
"""
import collections

import numpy as np
import torch

from . import _abi as A

Item = collections.namedtuple('Item', 'name kind dst dst_off bytes src src_off')
Item.__new__.__defaults__ = (None, 0)


def _row_bytes(t):
    """bytes of one slot's row of the per-slot tensor t [B, ...]"""
    return int(np.prod(t.shape[1:], dtype=np.int64)) * t.element_size()


def restore_items(env, prev_cells=None):
    """The ranges d2d_stream_restore puts back for a refilled slot of `env`, as Items over the env's tensors: exactly the buffers
    VecDrone2DEnv._refill_rest touches outside the masked resets -- the per-step outputs, the action, under RVO the velocities as
    state.init_rvo leaves them (zero for the k = min(agent_number, N) seeded agents, the preferred velocity out of the `agents`
    planes for the static map's cell agents), the plan statistics and the storage no reset covers (trajectory, boxes, search nodes
    and hash, the scratch half of the velocity swap), the Jerk_Primitive choice and status, with swept_obs the swept map, its
    crop and its count (include/d2d_swept.h), with seen_obs the time-since-observed map's records and the call of its latest update
    (include/d2d_seen.h), with scan_obs the rays of the latest step and its counter (include/d2d_scan.h) -- and `prev_cells`, the previous count
    of terms['explored'].  A buffer of no elements is left out."""
    s, items = env.state, []

    def zero(name, t, off=0, nbytes=None):
        nbytes = _row_bytes(t) if nbytes is None else nbytes
        if t is not None and t.numel() and nbytes:
            items.append(Item(name, A.RESTORE_ZERO, t, off, nbytes))

    for name in ('plan_ok', 'wp_valid', 'wp', 'hit', 'newly', 'obs_local', 'obs_yaw', 'rng_draws', 'action'):
        if s.t.get(name) is not None:
            zero(name, s.t[name])
    if env.rvo:
        N, k = env.cfg.N, min(int(env.params.agent_number), env.cfg.N)
        vel, agents = s.agent_vel, s.agents
        for axis, plane in (('x', A.A_VX), ('y', A.A_VY)):
            zero(f'agent_vel.{axis}[:k]', vel, (0 if axis == 'x' else N) * 8, k * 8)
        for axis, plane in (('x', A.A_VX), ('y', A.A_VY)):
            if N > k:
                items.append(Item(f'agent_vel.{axis}[k:]', A.RESTORE_COPY, vel, ((0 if axis == 'x' else N) + k) * 8, (N - k) * 8,
                                  agents, (plane * N + k) * 8))
    if env.plugins is not None:
        for name in ('plan_stat', 'traj', 'traj_box', 'nodes', 'hash'):
            zero(name, env.plugins.t[name])
    if env.rvo:
        zero('agent_vel_out', s.agent_vel_out)
    if env.jerk is not None:
        for name in ('choice', 'stat'):
            zero('jerk.' + name, env.jerk.t[name])
    if getattr(env, 'swept', None) is not None and len(env.swept) > 1:      # a rebuilt slot has a zero swept map at its step 0
        for name in ('map', 'obs', 'count'):
            zero('swept.' + name, env.swept[name])
    if getattr(env, 'seen', None) is not None:                              # ... and a map on which nothing has been seen yet
        for name in ('seen', 'last_call'):
            zero('seen.' + name, env.seen[name])
    if getattr(env, 'scan', None) is not None:                              # ... and no rays yet (include/d2d_scan.h)
        for name in A.SCAN_OUTPUTS:
            zero('scan.' + name, env.scan[name])
    if prev_cells is not None:
        zero('explored_prev', prev_cells)
    return items


def pack_items(items, device):
    """(uint8 tensor on `device` holding the d2d_restore_item array, the number of items).  Every range is checked against its
    tensor's row here: the library cannot look into device memory before a launch."""
    if len(items) > A.RESTORE_MAX_ITEMS:
        raise ValueError(f'd2d_stream_restore takes at most {A.RESTORE_MAX_ITEMS} items, got {len(items)}')
    arr = (A.RestoreItem * max(len(items), 1))()
    for rec, it in zip(arr, items):
        for t, off, what in ((it.dst, it.dst_off, 'dst'), (it.src, it.src_off, 'src')):
            if t is None:
                continue
            if not t.is_contiguous() or off < 0 or it.bytes < 0 or off + it.bytes > _row_bytes(t):
                raise ValueError(f'restore item {it.name!r}: {what} bytes [{off}, {off + it.bytes}) leave the slot\'s row of '
                                 f'{_row_bytes(t)} bytes, or the tensor is not contiguous')
        if it.kind not in (A.RESTORE_ZERO, A.RESTORE_COPY) or (it.kind == A.RESTORE_COPY) != (it.src is not None):
            raise ValueError(f'restore item {it.name!r}: kind {it.kind!r} (a copy names its source, a zero none)')
        rec.dst, rec.dst_stride, rec.dst_off = it.dst.data_ptr(), _row_bytes(it.dst), it.dst_off
        rec.src, rec.src_stride, rec.src_off = (it.src.data_ptr(), _row_bytes(it.src), it.src_off) if it.src is not None else (None, 0, 0)
        rec.bytes, rec.kind, rec.reserved = it.bytes, it.kind, 0
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device), len(items)


class ActionStream:
    """What VecDrone2DEnv.action_stream() returns.  `step(actions)` -> (obs, terms, done, info); `rows` [M, 8] int32 are the records
    runner.record_row reads (include/d2d_worlds_stream.h D2D_STREAM_R_*), written by the turn that follows an episode's last step;
    `finished` is the device scalar of the episodes harvested so far and `finished_now()` the one method that reads it."""

    def __init__(self, env, M, first, table, refill_every, max_attempts, capture=None):
        self.env, self.num_episodes, self.refill_every = env, M, max(1, int(refill_every))
        if capture is not None:
            capture.check_free(env)            # (refused before anything of the env is touched; owned only once the stream stands)
        self._m0, self._table = (first, None) if table is None else (None, table)
        B, dev, s = env.num_envs, env.device, env.state
        self.rows = env.stream_rows = torch.full((M, A.STREAM_ROW_F), -1, dtype=torch.int32, device=dev)
        env.steps_streamed = 0
        self.closed = False
        self.cells = torch.zeros(B, dtype=torch.int32, device=dev)
        self._prev = torch.zeros(B, dtype=torch.int32, device=dev)
        self.explored = torch.zeros(B, dtype=torch.int32, device=dev)
        self.live = torch.zeros(B, dtype=torch.bool, device=dev)
        self.goal = torch.zeros(B, dtype=torch.bool, device=dev)
        self._since = 0
        self._packed = {}                      # the velocity buffers swap every step under RVO: one packed list per parity
        self._idle = M == 0 or B == 0
        if self._idle:
            self.slot_episode = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
            if B:
                s.flags[:, A.F_DONE] = 1
                env._streamed = True
        else:
            self._up, self._ep, self._spec, self.slot_episode, self.refill, self.counts = env._stream_arrays(M, table, max_attempts)
            torch.eq(s.flags[:, A.F_DONE], 0, out=self.live)
        self.finished = self.counts[1]
        self.items = restore_items(env, self._prev)
        env._action_stream = self              # (load_slots() into an env with an open stream is refused)
        self.capture = capture                 # capture.Capture or None: the terminal frames of the slots a harvest records
        if capture is not None:
            capture.attach(env, self)          # last: a constructor that raised above leaves the capture free

    # ------------------------------------------------------------------ the turn
    def _item_array(self):
        s = self.env.state
        key = s.agent_vel.data_ptr() if self.env.rvo else 0
        if key not in self._packed:
            self.items = restore_items(self.env, self._prev)
            self._packed[key] = pack_items(self.items, self.env.device) + (self.items,)     # (the tensors outlive the launches)
        return self._packed[key][:2]

    def turn(self):
        """Queues the turn now if it is due (`refill_every` steps since the last one) and says whether it did.  step() does this
        itself at the start of the call, so a slot's terminal state stays readable until then.  A caller that wants the FIRST action of
        a fresh episode to come from that episode's own state calls turn() in front of its policy: the views of the previous result
        (observation, counters, info['episode'], info['steps']) then show the refilled slots at step 0 of their new episodes, the
        terminal state is gone, and the step() that follows does not turn again.  Otherwise the first action of a refilled slot is the
        one the caller computed from the old episode's last observation."""
        if self.closed:
            raise RuntimeError('ActionStream.turn(): the stream is closed')
        if self._idle or self._since < self.refill_every:
            return False
        self._since = 0
        env, b, s = self.env, self.env.backend, self.env.state
        if self.capture is not None:           # the finished slots as they ended, before the harvest lets them go
            self.capture.queue(self.slot_episode)
        b.stream_harvest(env.cfg, env._st, self.slot_episode, self.rows)
        if self._table is None:
            b.stream_assign(s.flags, self.num_episodes, self._m0, self.slot_episode, self._up['map_id'], self.refill, self.counts)
        else:
            ep = self._ep
            b.stream_assign_table(s.flags, ep[0], ep[1], ep[2], self.slot_episode, self._up['map_id'], self._up['env_par'],
                                  self._up['env_tgt'], self.refill, self.counts)
        b.build_worlds_masked(self._spec, env._st, self.refill)
        items, n = self._item_array()
        b.stream_restore(items, n, self.refill)
        env.reset_plugins(self.refill)
        env._seen_update()                     # a refilled slot's call 1 (its records are zero); every other slot's call has not moved
        env._tracks_update()                   # a refilled slot's counter jumped back and it has no active tracker: a zero window
        return True

    # ------------------------------------------------------------------ the surface
    def step(self, actions):
        """`actions`: [B] float64 on the env's device, in [-1, 1] as VecDrone2DEnv.step takes them.  Returns (obs, terms, done, info):
        `obs` the dict of step() as views; `terms` device tensors [B]: newly_tracked, explored (this step's increase of the slot's
        discovered cells; the first step of a fresh world counts from 0), collision (0 none, 1 static, 2 dynamic: the flags byte of
        the CSV row), goal, dead_lock, freezing, with seen_obs refreshed (VecDrone2DEnv.refreshed), with tracks_obs track_cells (VecDrone2DEnv.track_cells); `done` [B] bool; `info`: live (the slot played an episode in this step), episode
        (int32, the episode it played, -1 once retired), steps (the slot's step counter).  Everything but `done` is a view that the
        next call overwrites."""
        env, s = self.env, self.env.state
        if self.closed:
            raise RuntimeError('ActionStream.step(): the stream is closed')
        if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float64:
            raise TypeError(f'ActionStream.step(): actions is a float64 tensor on {env.device} (got '
                            f'{getattr(actions, "dtype", type(actions).__name__)}): the stream reads nothing from the host')
        if tuple(actions.shape) != (env.num_envs,) or actions.device != s.action.device:
            raise ValueError(f'ActionStream.step(): actions has shape {tuple(actions.shape)} on {actions.device}, the stream has '
                             f'[{env.num_envs}] slots on {s.action.device}')
        if self._idle:
            return self.result()
        self.turn()
        torch.eq(s.flags[:, A.F_DONE], 0, out=self.live)
        torch.where(self.live, actions, s.action, out=s.action)
        env._episode_steps(1)
        env.steps_streamed += 1
        self._since += 1
        env.backend.stream_explored(env.cfg, env._st, self.cells)
        torch.sub(self.cells, self._prev, out=self.explored)
        self._prev.copy_(self.cells)
        return self.result()

    def result(self):
        """(obs, terms, done, info) of the slots as they stand, without a step: before the first call every slot is at step 0 of
        its first episode"""
        env, s = self.env, self.env.state
        obs, _, done, _ = env._result()
        torch.eq(s.counters[:, A.C_SM], A.SM_GOAL_REACHED, out=self.goal)
        terms = {'newly_tracked': s.newly, 'explored': self.explored, 'collision': s.flags[:, A.F_COLLISION], 'goal': self.goal,
                 'dead_lock': s.flags[:, A.F_DEADLOCK], 'freezing': s.flags[:, A.F_FREEZING]}
        if env.seen is not None:               # the cells the slot's pose newly covered (include/d2d_seen.h)
            terms['refreshed'] = env.seen['refreshed']
        if env.tracks is not None:             # the cells of the slot's window a tracker's forecast reaches (include/d2d_tracks.h)
            terms['track_cells'] = env.tracks['cells']
        info = {'live': self.live, 'episode': self.slot_episode, 'steps': s.counters[:, A.C_STEPS]}
        return obs, terms, done, info

    def finished_now(self):
        """The episodes harvested so far, read from the device (a synchronisation).  An episode is harvested by the turn of the
        call after its last step, so a loop `while stream.finished_now() < M: stream.step(...)` ends"""
        return int(self.finished)

    def close(self):
        """Harvests the slots that finished since the last turn (so `rows` holds every episode that ended), synchronises and lets
        the stream's arrays go.  The env has then played other worlds than its snapshot: reset() refuses, as after stream_episodes()"""
        if self.closed:
            return
        if not self._idle:
            if self.capture is not None:
                self.capture.queue(self.slot_episode)
            self.env.backend.stream_harvest(self.env.cfg, self.env._st, self.slot_episode, self.rows)
        self.env.sync()
        if self.capture is not None:
            self.capture.detach(self)
        self.closed = True
        self.env._stream_keep = None
        self.env._action_stream = None
        self._packed = {}
