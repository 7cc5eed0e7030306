"""Episode driver with the reference's Experiment surface (experiment.py:26-106): builds env + gaze policy,
runs one episode, appends one CSV row with the reference's columns.  `main.py` of the reference does
`Experiment(cfg, result_dir).run()`; this is the same object on the accelerated env."""
import csv
import os

import numpy as np

from . import _abi as A
from .env import Drone2DEnv2
from .gaze import policy_list
from .params import with_defaults

CSV_COLUMNS = ['Method', 'Planner', 'Motion Profile', 'Map ID', 'Agent size', 'Number of agents', 'Number of pillars',
               'Agent speed', 'Drone speed', 'Depth variance', 'Initial position', 'Target position', 'Flight time',
               'Grid discovered', 'Agent tracked', 'Agent tracked time', 'Success', 'Static Collision',
               'Dynamic Collision', 'Freezing', 'Dead Lock', 'state machine']


class Experiment:
    def __init__(self, params, dir=None, device='cuda:0', backend=None):
        p = with_defaults(params)
        if p.gaze_method == 'NoControl':
            p.drone_view_range = 360                                   # experiment.py:28-29
        self.params = p
        self.env = Drone2DEnv2(p, device=device, backend=backend)
        self.dt = p.dt
        self.policy = policy_list[p.gaze_method]
        self.policy.__init__(self.policy, p)                           # class as instance, experiment.py:33-34
        self.result_dir = dir
        if dir and not os.path.isfile(dir) and p.record:
            with open(dir, 'w', newline='') as f:
                csv.writer(f).writerow(CSV_COLUMNS)

    def row(self, info):
        """The CSV row of experiment.py:73-103."""
        p = self.params
        n = len(info['tracker_buffer'])
        tracking_time = float(np.array([len(t.ts) * 0.1 for t in info['tracker_buffer']]).sum())
        gm = info['drone'].map.grid_map
        with np.errstate(divide='ignore', invalid='ignore'):
            mean_time = np.float64(tracking_time) / n if n else float('nan')
        return (p.gaze_method, p.planner, p.motion_profile, p.map_id, p.agent_radius, p.agent_number,
                p.pillar_number, p.agent_max_speed, p.drone_max_speed, p.var_cam, p.init_position, p.target_list[0],
                info['flight_time'], gm.shape[0] * gm.shape[1] - np.sum(np.where(gm == 0, 1, 0)), n, mean_time,
                1 if info['state_machine'] == A.SM_GOAL_REACHED else 0, 1 if info['collision_flag'] == 1 else 0,
                1 if info['collision_flag'] == 2 else 0, info['freezing_flag'], info['dead_lock_flag'],
                info['state_machine'])

    def run(self):
        self.env.reset()
        done, info = False, self.env.info
        while not done:
            a = self.policy.plan(self.policy, self.env.info)
            _, _, done, info = self.env.step(0.0 if a is None else a)
        row = self.row(info)
        if self.params.record and self.result_dir:
            with open(self.result_dir, 'a', newline='') as f:
                csv.writer(f).writerow(row)
        return row


def batch_records(env):
    """[B, 8] int64 numpy: per env the numbers its CSV row is made of, in the columns of include/d2d_worlds_stream.h
    (D2D_STREAM_R_*): C_STEPS, C_SM, C_BUF_N, C_BUF_TS, flags[0..2] and the number of non-zero cells of dmap -- what
    d2d_stream_harvest records for a finished slot."""
    s = env.state
    c = s.counters.cpu().numpy()
    f = s.flags.cpu().numpy()
    disc = (s.dmap != 0).flatten(1).sum(1).cpu().numpy()
    out = np.zeros((env.num_envs, A.STREAM_ROW_F), dtype=np.int64)
    out[:, [A.STREAM_R_STEPS, A.STREAM_R_SM, A.STREAM_R_BUF_N, A.STREAM_R_BUF_TS]] = c[:, [A.C_STEPS, A.C_SM, A.C_BUF_N, A.C_BUF_TS]]
    out[:, A.STREAM_R_FLAG0:A.STREAM_R_FLAG0 + 3] = f[:, :3]
    out[:, A.STREAM_R_DMAP] = disc
    return out


def record_row(params, map_id, rec):
    """The tuple with the columns of experiment.py:73-103 of one record (batch_records / d2d_stream_harvest) of the world `map_id`."""
    p = params
    n = int(rec[A.STREAM_R_BUF_N])
    tracking_time = float(rec[A.STREAM_R_BUF_TS]) * 0.1
    with np.errstate(divide='ignore', invalid='ignore'):
        mean_time = np.float64(tracking_time) / n if n else float('nan')
    sm = int(rec[A.STREAM_R_SM])
    f = rec[A.STREAM_R_FLAG0:A.STREAM_R_FLAG0 + 3]
    return (p.gaze_method, p.planner, p.motion_profile, map_id, p.agent_radius,
            p.agent_number, p.pillar_number, p.agent_max_speed, p.drone_max_speed, p.var_cam, p.init_position,
            p.target_list[0], int(rec[A.STREAM_R_STEPS]) * p.dt, int(rec[A.STREAM_R_DMAP]), n, mean_time,
            1 if sm == A.SM_GOAL_REACHED else 0, 1 if f[0] == 1 else 0, 1 if f[0] == 2 else 0,
            int(f[2]), int(f[1]), sm)


def study_row(params, rec, agent_speed=None):
    """record_row for an episode of a table (EpisodeStream(episodes=...), ValidationStudy): `params` is the episode's own Params, so
    the map id, the start and the target of the row are the episode's.  `agent_speed`: the 'Agent speed' column where it is not
    agent_max_speed -- script/validation_speed.py:159 writes -1 for its redrawn velocities."""
    row = record_row(params, params.map_id, rec)
    return row if agent_speed is None else row[:7] + (agent_speed,) + row[8:]


def batch_rows(params, env):
    """One tuple per env of VecDrone2DEnv `env` with the columns of experiment.py:73-103, read off the state as its episodes left it."""
    rec = batch_records(env)
    return [record_row(params, params.map_id + env.env_offset + e, rec[e]) for e in range(env.num_envs)]


class _BatchRows:
    """rows() / write_csv() of a batch whose envs have played one episode each (self.params, self.env)."""

    def rows(self):
        """One tuple per env with the columns of experiment.py:73-103."""
        return batch_rows(self.params, self.env)

    def write_csv(self, path):
        new = not os.path.isfile(path)
        with open(path, 'a', newline='') as fh:
            w = csv.writer(fh)
            if new:
                w.writerow(CSV_COLUMNS)
            w.writerows(self.rows())


class ExperimentBatch(_BatchRows):
    """The reference's sweep of episodes (`main.py:26-57`: the same cfg over many map ids, one Experiment and one
    CSV row each) as ONE device batch: env i is the world of `map_id + i`, the gaze policy and the planner run on
    the device (Oxford / LookAhead / LookGoal / Owl / Primitive), every env plays exactly one episode (`D2D_DONE_FREEZE`)
    and `rows()` returns the reference's CSV rows.  Everything an episode needs stays on the GPU; the host only reads
    the rows.

    `LookAhead` (main.py:10's default method) and `LookGoal` run as the device gaze stage (yaw_planner.py:28-39,
    :225-257 with a bit-exact restatement of `math.atan2`), one `closed_loop` call per chunk like Oxford.  On a backend
    without that stage (`supports_device_heading_gaze`, e.g. the CPU oracle) LookAhead runs from the host instead: every
    step pulls the drone's velocity and yaw, evaluates the policy with the host's libm and uploads the actions -- one
    launch per step instead of one per episode; LookGoal is refused there.  `device_gaze=False` takes that host path for
    LookAhead on any backend (A/B measurements).  `Owl` (yaw_planner.py:151-222) runs as a device gaze stage too and is refused
    on a backend without it (`supports_device_owl_gaze`).  `device_worlds=True`: the seeded worlds are built by the device too
    (include/d2d_worlds.h) instead of by `workers` host processes."""

    def __init__(self, params, num_envs, device='cuda:0', backend=None, workers=0, device_gaze=True, device_worlds=False):
        from .vec_env import VecDrone2DEnv, build_worlds
        p, self._host_lookahead = self.accepted(params, backend, device_gaze)
        self.params = p
        worlds = 'device' if device_worlds else build_worlds(p, num_envs, workers=workers)
        self.env = VecDrone2DEnv(p, num_envs, device=device, backend=backend, planner=p.planner, worlds=worlds,
                                 device_plugins=True, gaze='external' if self._host_lookahead else p.gaze_method)
        self.max_steps = int(np.ceil(p.max_flight_time / p.dt)) + 1           # freezing ends every episode by then

    @staticmethod
    def accepted(params, backend=None, device_gaze=True):
        """(the Params this runner plays, does LookAhead run from the host?), or the runner's refusal"""
        from ._lib import HipBackend
        p = with_defaults(params)
        if p.planner == 'Jerk_Primitive':
            raise NotImplementedError("ExperimentBatch: planner 'Jerk_Primitive' does not run inside the persistent closed loop (its "
                                      'stage lives in libd2d_jerk.so); step a VecDrone2DEnv(..., planner=\'Jerk_Primitive\', '
                                      'device_plugins=True) with step(), or run the episodes through runner.Experiment, one at a time.  '
                                      'runner.SteppedExperimentBatch plays the episodes of this planner as a batch')
        if p.gaze_method not in ('Oxford', 'Rotating', 'NoControl', 'LookAhead', 'LookGoal', 'Owl') or p.planner not in ('Primitive', 'NoMove'):
            raise NotImplementedError('ExperimentBatch runs the device plugins: gaze_method Oxford / LookAhead / LookGoal / Owl / '
                                      'Rotating / NoControl, planner Primitive / NoMove (use Experiment, one episode at a time, for '
                                      'other host plugin classes)')
        if p.motion_profile == 'RVO':
            raise NotImplementedError("ExperimentBatch: motion_profile 'RVO' does not run inside the persistent closed loop (its stage "
                                      'lives in libd2d_rvo.so); SteppedExperimentBatch plays the episodes of planner Primitive '
                                      'under it as a batch (Experiment, one episode at a time, runs everything else)')
        device_heading = device_gaze and getattr(backend if backend is not None else HipBackend, 'supports_device_heading_gaze', False)
        if p.gaze_method == 'LookGoal' and not device_heading:
            raise NotImplementedError('ExperimentBatch: LookGoal needs a backend with the device LookAhead / LookGoal stage')
        if p.gaze_method == 'Owl' and not getattr(backend if backend is not None else HipBackend, 'supports_device_owl_gaze', False):
            raise NotImplementedError('ExperimentBatch: Owl needs a backend with the device Owl stage (use Experiment with the host '
                                      'policy gaze.Owl, one episode at a time)')
        host_lookahead = p.gaze_method == 'LookAhead' and not device_heading
        if p.gaze_method == 'NoControl':
            p.drone_view_range = 360                                   # experiment.py:28-29
        return p, host_lookahead

    def _lookahead_actions(self):
        """yaw_planner.LookAhead.plan for every env (gaze.LookAhead, vectorised over the batch on the host): the path of a
        backend without the device stage."""
        from .gaze import _yaw_rate_towards
        import math
        p = self.params
        d = self.env.state.drone[:, [A.D_VX, A.D_VY, A.D_YAW]].cpu().numpy()
        out = np.zeros(len(d))
        for e, (vx, vy, yaw) in enumerate(d):
            if vx != 0 or vy != 0:
                out[e] = _yaw_rate_towards(math.degrees(math.atan2(-vy, vx)) % 360, yaw, p.dt, p.drone_max_yaw_speed)
        return out

    def run(self, chunk=None):
        n = self.max_steps
        if self._host_lookahead:
            for t in range(n):
                self.env._set_action(self._lookahead_actions())
                self.env.closed_loop(1, freeze_done=True)
                if t % 16 == 15 and bool(self.env.state.flags[:, A.F_DONE].all()):
                    break
            self.env.sync()
            return self.rows()
        chunk = chunk or n
        for c0 in range(0, n, chunk):
            self.env.closed_loop(min(chunk, n - c0), freeze_done=True)
        self.env.sync()
        return self.rows()


STEPPED_GAZE_METHODS = ('LookAhead', 'Owl', 'LookGoal', 'Oxford', 'Rotating', 'NoControl')


class SteppedExperimentBatch(_BatchRows):
    """ExperimentBatch for `planner='Jerk_Primitive'`: the `Jerk_Primitive` half of the reference's validation sweeps
    (script/validation_shape.py, validation_speed.py: planners x gaze methods x map ids) as device batches.  Env i is the world of
    `map_id + i`; every env plays exactly one episode and `rows()` returns the reference's CSV rows.

    The planner's stage lives in a library of its own, so the episodes do not run inside the persistent closed loop but over
    `VecDrone2DEnv.run_episodes`: per step the gaze launch (include/d2d_gaze.h), the RVO launches under `motion_profile='RVO'`, the
    first half of the step, the plan (include/d2d_jerk.h), the second half; finished envs are frozen (D2D_ST_SKIP_DONE) and the host
    looks at the flags once every `check_every` steps.  Every `--gaze_method` name runs: LookAhead and Owl as that launch, Rotating
    and NoControl as constants, and LookGoal and Oxford as the constant 0 they are under this planner (its trajectory is empty at
    every policy call; Oxford's own maps are therefore not kept).  On a backend with the launches of include/d2d_jerk_live.h and
    d2d_rvo_live.h (the HIP backend) every launch leaves finished envs alone and a finished env is frozen in everything; on one
    without them the plan's outputs and tracker bookkeeping (under RVO its agents) go on changing, which is nothing a row reads
    (VecDrone2DEnv.run_episodes, `live`).  `jerk_tie`: as in VecDrone2DEnv.

    `planner='Primitive'` under `motion_profile='RVO'` runs here too (under CVM it stays with ExperimentBatch): the plugins of
    libd2d_hip.so as stages that leave finished envs alone (include/d2d_stepped.h) around the RVO launches that do the same
    (include/d2d_rvo_live.h), with Oxford, LookAhead, LookGoal and Owl as the device gaze stage.  There a finished env is frozen in
    everything, its agents, their velocities and its plugin state included."""

    def __init__(self, params, num_envs, device='cuda:0', backend=None, workers=0, device_worlds=False, jerk_tie=None):
        from .vec_env import VecDrone2DEnv, build_worlds
        self.params = p = self.accepted(params, backend)
        worlds = 'device' if device_worlds else build_worlds(p, num_envs, workers=workers)
        self.env = VecDrone2DEnv(p, num_envs, device=device, backend=backend, planner=p.planner, worlds=worlds,
                                 device_plugins=True, gaze=p.gaze_method, jerk_tie=jerk_tie)
        self.max_steps = int(np.ceil(p.max_flight_time / p.dt)) + 1           # freezing ends every episode by then
        self.steps_run = 0

    @staticmethod
    def accepted(params, backend=None):
        """the Params this runner plays, or the runner's refusal"""
        from ._lib import HipBackend
        p = with_defaults(params)
        primitive_rvo = p.planner == 'Primitive' and p.motion_profile == 'RVO'     # each (planner, profile) cell has one batch runner
        if p.planner != 'Jerk_Primitive' and not primitive_rvo:
            raise NotImplementedError(f"SteppedExperimentBatch runs planner 'Jerk_Primitive' (got {p.planner!r}), and planner "
                                      "'Primitive' under motion_profile 'RVO'; ExperimentBatch runs Primitive and NoMove inside the "
                                      'persistent closed loop')
        if p.gaze_method not in STEPPED_GAZE_METHODS:
            raise NotImplementedError(f'SteppedExperimentBatch: gaze_method {p.gaze_method!r}: ' + ' / '.join(STEPPED_GAZE_METHODS) +
                                      ' (use Experiment, one episode at a time, for other host plugin classes)')
        have = lambda flag: getattr(backend if backend is not None else HipBackend, flag, False)   # noqa: E731
        if primitive_rvo and not (have('supports_stepped_plugins') and have('supports_rvo_live')):
            raise NotImplementedError("SteppedExperimentBatch: planner 'Primitive' under motion_profile 'RVO' needs a backend with the "
                                      'stages and RVO launches that leave finished envs alone (include/d2d_stepped.h, d2d_rvo_live.h)')
        if not primitive_rvo and not have('supports_step_gaze'):
            raise NotImplementedError("SteppedExperimentBatch needs a backend with the step path's gaze launch (include/d2d_gaze.h)")
        if p.gaze_method == 'NoControl':
            p.drone_view_range = 360                                   # experiment.py:28-29
        return p

    def run(self, check_every=16):
        self.steps_run = self.env.run_episodes(self.max_steps, check_every)
        self.env.sync()
        return self.rows()


class EpisodeStream:
    """`num_episodes` seeded episodes (map ids `map_id + 0 .. map_id + num_episodes - 1`) streamed through `slots` resident envs
    (VecDrone2DEnv.stream_episodes): a slot whose episode has ended is handed the next map id and rebuilt in place on the device
    (include/d2d_worlds_stream.h), so memory is bounded by the slots and no slot waits for the slowest episode of a batch.

    The env is the one the batch runner of `params`' cell would build with device worlds -- ExperimentBatch's for Primitive / NoMove
    under CVM (the persistent closed loop), SteppedExperimentBatch's for Jerk_Primitive and for Primitive under RVO -- and that
    runner's refusals hold here.  `rows()` are its rows: an episode depends on nothing but its world, so neither the slot that
    played it nor `refill_every` can change its row, and the rows come out in episode order.  An episode whose world could not be
    placed (column 0 of its record == STREAM_BUILD_FAILED, `build_failed` lists their map ids) has a row of zeros."""

    def __init__(self, params, num_episodes=None, slots=None, device='cuda:0', backend=None, jerk_tie=None, episodes=None,
                 redraw_agents=False, agent_speed=None, capture=None):
        """`episodes`: a table in place of consecutive map ids (VecDrone2DEnv.stream_episodes): a list of Params, or of (map_id,
        init_position, target_list) triples over `params`; episode k is the world of row k and `rows()` carries the row's map id,
        start and target.  The env is built from the first rows, so they are the envs as constructed.  `redraw_agents`: every world
        is that of the validation study, the agents' preferred velocities redrawn behind the construction; `agent_speed`: the rows'
        'Agent speed' column where it is not agent_max_speed (study_row).  `capture`: a callable env -> capture.Capture (the
        env is built here), or None: with params.record_img set and gaze_method != 'NoControl', the reference's condition
        (envs/training_v3.py:180-187), Capture(env, ('static', 'dynamic')).  run() saves the gallery into params.img_dir under that
        condition and no other, whoever made the capture: a caller's capture without record_img, or under NoControl, is filled and
        left to the caller (`self.capture`)."""
        from .vec_env import VecDrone2DEnv, build_worlds_device_of, table_params
        if slots is None or (num_episodes is None) == (episodes is None):
            raise TypeError('EpisodeStream(params, num_episodes, slots) or EpisodeStream(params, episodes=[...], slots=B)')
        p = with_defaults(params)
        record = bool(getattr(p, 'record_img', False)) and p.gaze_method != 'NoControl'
        stepped = p.planner == 'Jerk_Primitive' or (p.planner == 'Primitive' and p.motion_profile == 'RVO')
        if stepped:
            p = SteppedExperimentBatch.accepted(p, backend)
        else:
            p, host_lookahead = ExperimentBatch.accepted(p, backend)
            if host_lookahead:
                raise NotImplementedError('EpisodeStream: LookAhead needs a backend with the device LookAhead / LookGoal stage (a '
                                          'streamed episode has no host policy); ExperimentBatch drives it from the host')
        self.params, self.num_episodes = p, int(num_episodes) if episodes is None else len(episodes)
        self.episodes, self.agent_speed = None, agent_speed
        worlds = 'device'
        if episodes is not None:
            from ._lib import backend_for
            backend = backend_for(backend, device)
            rows = [ep if isinstance(ep, (tuple, list)) else self._accepted_row(ep, p) for ep in episodes]
            self.episodes = rows
            # the env's slots are the first rows; surplus slots (fewer episodes than slots) hold the last row's world and are
            # retired before the first step
            first = table_params(p, rows[:int(slots)]) if rows else [p]
            first += [first[-1]] * (int(slots) - len(first))
            worlds = build_worlds_device_of(first, device, backend, redraw=redraw_agents) if int(slots) else 'device'
        self.env = VecDrone2DEnv(p, int(slots), device=device, backend=backend, planner=p.planner, worlds=worlds,
                                 device_plugins=True, gaze=p.gaze_method, jerk_tie=jerk_tie if stepped else None,
                                 redraw_agents=redraw_agents)
        self.max_steps = int(np.ceil(p.max_flight_time / p.dt)) + 1
        self.steps_run = 0
        self.records = None
        self.capture, self.image_paths, self._record = None, [], record
        if capture is not None:
            self.capture = capture(self.env)
        elif record and int(slots):
            from .capture import Capture
            self.capture = Capture(self.env, ('static', 'dynamic'))

    @staticmethod
    def _accepted_row(ep, p):
        """a Params row as the runner plays it: the one change the batch runners make to their Params (experiment.py:28-29)"""
        q = with_defaults(ep)
        if p.gaze_method == 'NoControl' and q.gaze_method == 'NoControl':
            q.drone_view_range = 360
        return q

    def run(self, refill_every=64, **kw):
        if self.records is not None:
            raise RuntimeError('EpisodeStream.run(): this stream has run, and its slots hold the last worlds that passed through them; '
                               'rows() returns its rows again, a new EpisodeStream runs the episodes again')
        if self.episodes is not None:
            kw['episodes'] = self.episodes
        if self.capture is not None:
            kw['capture'] = self.capture
        self.records = self.env.stream_episodes(None if self.episodes is not None else self.num_episodes, refill_every, **kw).cpu().numpy()
        self.steps_run = self.env.steps_streamed
        if self.capture is not None and self._record:     # the reference's condition, for a capture of the caller's making too
            self.image_paths = self.capture.save(self.params.img_dir)
        return self.rows()

    @property
    def build_failed(self):
        """map ids of the episodes whose world hit max_attempts"""
        failed = np.nonzero(self.records[:, A.STREAM_R_STEPS] == A.STREAM_BUILD_FAILED)[0]
        if self.episodes is not None:
            ps = self.env.episode_params(self.episodes)
            return [int(ps[int(k)].map_id) for k in failed]
        m0 = self.params.map_id + self.env.env_offset
        return [m0 + int(k) for k in failed]

    def rows(self):
        """One tuple per episode, in episode order, with the columns of experiment.py:73-103."""
        if self.records is None:
            raise RuntimeError('EpisodeStream.rows(): run() first')
        if self.episodes is not None:
            ps = self.env.episode_params(self.episodes)
            return [study_row(ps[k], self.records[k], self.agent_speed) for k in range(self.num_episodes)]
        m0 = self.params.map_id + self.env.env_offset
        return [record_row(self.params, m0 + k, self.records[k]) for k in range(self.num_episodes)]

    write_csv = _BatchRows.write_csv


STUDY_AXIS = (40, 250, 460)          # validation_*.py: axis_range


def study_pairs():
    """The 72 (start, target) pairs of a study cell in the scripts' order: product(product(axis, axis), product(axis, axis)) with
    start != target (validation_speed.py:118-121)"""
    from itertools import product
    return [(s, t) for s, t in product(product(STUDY_AXIS, STUDY_AXIS), product(STUDY_AXIS, STUDY_AXIS)) if s != t]


class ValidationStudy:
    """The reference's validation study -- the runs the difficulty metrics exist for -- with the scripts' loops as data.

    kind 'speed'  script/validation_speed.py: agent_number x agent_radius (5, 10, 15) at the default agent speed, map ids 0 .. 4,
                  drone_max_speed (20, 40, 60), (planner, gaze) = ('Primitive', 'Oxford'); after env.reset() every agent's preferred
                  velocity is redrawn (host_init.redraw_agent_velocities, D2D_WE_REDRAW) and the row's 'Agent speed' is the
                  script's -1.  The script's other pair, ('MPC', 'LookAhead'), is skipped: MPC is out of scope.
    kind 'size'   script/validation_size.py: agent_number x agent_max_speed (20, 40, 60) at agent_radius = -1, the same maps and
                  drone speeds, ('Jerk_Primitive', 'NoControl') through Experiment.run: nothing is redrawn there, and the row is
                  experiment.py's.

    A cell is (agent number, agent size or speed, drone speed, planner, gaze): everything a stream shares.  Its table is 5 maps x
    72 (start, target) pairs = 360 episodes, maps outermost as in the scripts (which loop the maps outside the drone speeds: the
    rows are the same, in another order).  `cells()` yields (cell, Params, table of Params); `run()` streams each cell through
    `slots` resident envs (EpisodeStream(episodes=...)) and returns the reference's CSV rows, or writes them to `path`.

    script/validation_shape.py redraws nothing and needs only a label-grid path per cell, which `static_map` takes
    (host_init.load_static_map loads any .npy): such a cell is an EpisodeStream(episodes=...) like any other.  Generating its random
    maps stays with the reference."""

    KINDS = {
        'speed': dict(second='agent_radius', values=(5, 10, 15), pairs=(('Primitive', 'Oxford'),), redraw=True, agent_speed=-1,
                      fixed={}),
        'size': dict(second='agent_max_speed', values=(20, 40, 60), pairs=(('Jerk_Primitive', 'NoControl'),), redraw=False,
                     agent_speed=None, fixed=dict(agent_radius=-1)),
    }

    def __init__(self, kind, agent_numbers=(10, 20, 30), drone_max_speeds=(20, 40, 60), map_ids=range(5), **params_kw):
        if kind not in self.KINDS:
            raise ValueError(f"ValidationStudy: kind {kind!r}: 'speed' or 'size'")
        self.kind, self.spec = kind, self.KINDS[kind]
        self.agent_numbers, self.drone_max_speeds, self.map_ids = tuple(agent_numbers), tuple(drone_max_speeds), tuple(map_ids)
        self.params_kw = params_kw                      # e.g. max_flight_time, static_map: the same for every cell

    def cells(self):
        """(cell, Params, episodes) per cell: cell = (agent number, agent size or speed, drone speed, planner, gaze), Params the
        stream's, episodes the table of len(map_ids) * 72 Params"""
        import copy
        from itertools import product
        from .params import Params
        sp = self.spec
        for n, v in product(self.agent_numbers, sp['values']):
            for d, (planner, gaze) in product(self.drone_max_speeds, sp['pairs']):
                kw = dict(self.params_kw, agent_number=n, drone_max_speed=d, planner=planner, gaze_method=gaze, debug=False, **sp['fixed'])
                kw[sp['second']] = v
                base = Params(**kw)
                table = []
                for m in self.map_ids:
                    for start, target in study_pairs():
                        p = copy.copy(base)
                        p.map_id, p.init_position, p.target_list = m, start, [target]
                        table.append(p)
                yield (n, v, d, planner, gaze), (table[0] if table else base), table

    def run(self, slots=64, path=None, device='cuda:0', backend=None, refill_every=64, cells=None):
        """Streams every cell (or those of `cells`, a list of cell tuples) and returns all rows; `path`: also appended there as CSV"""
        rows = []
        for cell, p, table in self.cells():
            if cells is not None and cell not in cells:
                continue
            xs = EpisodeStream(p, episodes=table, slots=min(int(slots), len(table)), device=device, backend=backend,
                               redraw_agents=self.spec['redraw'], agent_speed=self.spec['agent_speed'])
            got = xs.run(refill_every=refill_every)
            if path:
                xs.write_csv(path)
            rows += got
        return rows
