"""Test-side backends for whole episode streams without a GPU (VecDrone2DEnv.stream_episodes, runner.EpisodeStream): the
launches of include/d2d_worlds_stream.h, and d2d_worlds_build itself, restated in numpy (tests/stream_model.py) over the CPU backends
that play batched episodes -- stepped_backend.SteppedOracleBackend for the Primitive plugins under either motion profile,
jerk_live_backend.LiveJerkBackend for Jerk_Primitive.  Test infrastructure: the product package never imports this.

The worlds are host_init.init_world of `params`, so a backend is made for one Params (map_id aside).  harvest and assign read the
env's tensors: one backend per env, `attach(env)` after the env is built (stream_of does both).  A world is only checked against
`max_attempts` where a test lowers it: the answer comes from the sequential host form of the device construction
(tests/csrc/world_host.c), since init_world, like the reference, would loop for ever."""
import copy
import tempfile

import numpy as np

import stream_model as SM
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend

_WORLD_HOST = None


def _capped(pkg, params, map_id, max_attempts):
    global _WORLD_HOST
    if _WORLD_HOST is None:
        import world_cases
        _WORLD_HOST = world_cases.build_world_host(tempfile.mkdtemp(prefix='stream_world_host_'))[1]
    p = copy.copy(params)
    p.map_id = int(map_id)
    return bool(_WORLD_HOST(pkg, [p], max_attempts=max_attempts)['status'][0])


class _Stream:
    supports_device_worlds = True
    supports_episode_stream = True
    params = None

    def of(self, params):
        from drone2d_amd.params import with_defaults
        self.params = with_defaults(params)
        return self

    def _build(self, spec, st, slots, flags):
        import drone2d_amd as pkg
        v = SM.world_views(spec, st)
        for e in slots:
            m = int(v['map_id'][e])
            capped = spec.max_attempts != A.WORLDS_MAX_ATTEMPTS and _capped(pkg, self.params, m, spec.max_attempts)
            SM.load_world(v, e, None if capped else SM.world_of(self.params, m), spec.grid_tile, flags)

    def build_worlds(self, spec, st):
        self._build(spec, st, range(spec.B), False)

    def build_worlds_masked(self, spec, st, refill):
        self._build(spec, st, np.nonzero(refill.numpy())[0], True)

    def stream_clear(self, t, refill):
        t[refill.bool()] = 0

    def stream_harvest(self, cfg, st, slot_episode, rows):
        from drone2d_amd import runner
        SM.harvest(runner.batch_records(self.env), self.env.state.flags.numpy(), slot_episode.numpy(), rows.numpy())

    def stream_assign(self, flags, num_episodes, map_id0, slot_episode, map_id, refill, counts):
        SM.assign(flags.numpy(), slot_episode.numpy(), map_id.numpy().view(np.uint32), refill.numpy(), counts.numpy(), int(num_episodes),
                  int(map_id0))


class StreamPrimitiveBackend(_Stream, SteppedOracleBackend):
    name = 'oracle+rvo_host+live+stream'


class StreamJerkBackend(_Stream, LiveJerkBackend):
    name = 'oracle+jerk_host+gaze_host+rvo_host+live+stream'


def backend_for_params(params):
    return (StreamJerkBackend if params.planner == 'Jerk_Primitive' else StreamPrimitiveBackend)().of(params)


def stream_of(params, num_episodes, slots, **kw):
    """runner.EpisodeStream of `params` on a fresh stream backend, attached"""
    from drone2d_amd import runner
    backend = backend_for_params(params)
    xs = runner.EpisodeStream(params, num_episodes, slots, device='cpu', backend=backend, **kw)
    backend.attach(xs.env)
    return xs


def batch_of(params, num_envs):
    """the batch runner of the same cell on its usual CPU backend, host-built worlds"""
    from drone2d_amd import runner
    stepped = params.planner == 'Jerk_Primitive' or params.motion_profile == 'RVO'
    backend = (LiveJerkBackend if params.planner == 'Jerk_Primitive' else SteppedOracleBackend)()
    xb = (runner.SteppedExperimentBatch if stepped else runner.ExperimentBatch)(params, num_envs, device='cpu', backend=backend)
    backend.attach(xb.env)
    return xb


def same_rows(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((u != u and v != v) or u == v for u, v in zip(x, y)) for x, y in zip(a, b))
