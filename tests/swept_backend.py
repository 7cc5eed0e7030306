"""Test-side backend for swept_obs=True without a GPU: tests/stepped_backend.SteppedOracleBackend (through the action-stream backends
of tests/action_stream_backend.py, so that streams run on it too) plus the two launches of include/d2d_swept.h done by
tests/swept_model.py on the attached env's tensors.  The CPU stand-in the other libraries' *_backend.py files are.  Test
infrastructure: the product package never imports this."""
import numpy as np
import torch

import action_stream_backend as AB
import swept_model as SW
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend


class _Swept:
    supports_swept_obs = True

    def swept_mark(self, cfg, st, plan, sw):
        env = self.env
        assert sw is env._swept and cfg.grid_tile == 0
        done = env.state.flags[:, A.F_DONE].numpy() != 0
        env.swept['live'].copy_(torch.from_numpy((~done).astype(np.uint8)))
        for e in np.nonzero(~done)[0]:
            full, m = SW.mark_env(env, int(e))
            env.swept['map'][e] = torch.from_numpy(full)
            env.swept['count'][e] = m

    def swept_crop(self, cfg, st, sw):
        env = self.env
        for e in np.nonzero(env.swept['live'].numpy())[0]:
            env.swept['obs'][e] = torch.from_numpy(SW.crop(env.swept['map'][e].numpy(), env.state.drone[e, :2].numpy(), cfg))


class SweptOracleBackend(_Swept, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+swept'


class SweptTurnBackend(_Swept, AB.TurnPrimitiveBackend):
    name = AB.TurnPrimitiveBackend.name + '+swept'


class SweptJerkBackend(_Swept, LiveJerkBackend):
    """Jerk_Primitive: the channel is a resident zero tensor and neither launch is ever queued"""
    name = LiveJerkBackend.name + '+swept'

    def swept_mark(self, *a):
        raise AssertionError('Jerk_Primitive queues no swept launch')

    swept_crop = swept_mark


def env_of(params, B, backend=None, **kw):
    """VecDrone2DEnv of `params` (host-built worlds unless `worlds` says otherwise) with the caller's gaze on a fresh backend, attached"""
    from drone2d_amd import vec_env
    backend = backend or SweptOracleBackend()
    kw.setdefault('gaze', 'external')
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, planner=params.planner, device_plugins=True, **kw)
    return backend.attach(env) if hasattr(backend, 'attach') else env
