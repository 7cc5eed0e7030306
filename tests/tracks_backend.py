"""Test-side backend for tracks_obs=True without a GPU: the launch of include/d2d_tracks.h done by tests/tracks_model.py on the host
memory behind the structs' pointers (so it needs no env attached: the constructor queues the first update itself), mixed into the
oracle backends of the other test modules.  The CPU stand-in the other libraries' *_backend.py files are.  Test infrastructure: the
product package never imports this."""
import numpy as np

import action_stream_backend as AB
import obs_channels_backend as OB
import stream_model as SM
import tracks_model as TM
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend


class _Tracks:
    supports_tracks_obs = True
    tracks_updates = 0

    def tracks_update(self, cfg, st, w):
        B, N, L = cfg.B, cfg.N, cfg.L
        drone, counters = SM.at(st.drone, (B, A.DF), np.float64), SM.at(st.counters, (B, A.CF), np.int32)
        win, cells, last = SM.at(w.win, (B, L, L), np.uint8), SM.at(w.cells, (B,), np.int32), SM.at(w.last_step, (B,), np.int32)
        self.tracks_updates += 1
        if N:
            kf, active = SM.at(st.kf, (B, N, A.KF), np.float64), SM.at(st.active, (B, N), np.uint8)
            radius = SM.at(w.trk_radius, (B, N), np.float64)
        for e in range(B):
            none = np.zeros((0, 4))
            out = TM.update(win[e], cells[e], last[e], counters[e, A.C_STEPS], drone[e], kf[e] if N else none, active[e] if N else none[:, 0],
                            radius[e] if N else none[:, 0], cfg, w.margin, w.samples, w.force)
            if out is not None:
                win[e], cells[e], last[e] = out


class TracksOracleBackend(_Tracks, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+tracks'


class TracksTurnBackend(_Tracks, AB.TurnPrimitiveBackend):
    name = AB.TurnPrimitiveBackend.name + '+tracks'


class TracksTurnJerkBackend(_Tracks, AB.TurnJerkBackend):
    name = AB.TurnJerkBackend.name + '+tracks'


class TracksJerkBackend(_Tracks, LiveJerkBackend):
    name = LiveJerkBackend.name + '+tracks'


class AllOracleBackend(_Tracks, OB.ChannelsOracleBackend):
    """all four observation channels on one env"""
    name = OB.ChannelsOracleBackend.name + '+tracks'


def backend_for(params):
    return (TracksJerkBackend if params.planner == 'Jerk_Primitive' else TracksOracleBackend)()


def stream_backend_for(params):
    return (TracksTurnJerkBackend if params.planner == 'Jerk_Primitive' else TracksTurnBackend)().of(params)


def env_of(params, B, backend=None, **kw):
    """VecDrone2DEnv of `params` (host-built worlds unless `worlds` says otherwise) with the caller's gaze on a fresh backend, attached"""
    from drone2d_amd import vec_env
    backend = backend or backend_for(params)
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', params.planner)
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, **kw)
    return backend.attach(env) if hasattr(backend, 'attach') else env
