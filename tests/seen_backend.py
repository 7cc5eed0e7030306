"""Test-side backend for seen_obs=True without a GPU: the launch of include/d2d_seen.h done by tests/seen_model.py on the host memory
behind the structs' pointers (so it needs no env attached: the constructor queues the first update itself), mixed into the oracle
backends of the other test modules.  The CPU stand-in the other libraries' *_backend.py files are.  Test infrastructure: the product
package never imports this."""
import numpy as np

import action_stream_backend as AB
import seen_model as SN
import stream_model as SM
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend


class _Seen:
    supports_seen_obs = True
    seen_view_range = None             # drone_view_range of the env's Params (env_of sets it; the stream backends hold .params)
    seen_updates = 0

    def seen_update(self, cfg, st, w):
        view_range = self.seen_view_range if self.seen_view_range is not None else self.params.drone_view_range
        B, W, H, L, n = cfg.B, cfg.W, cfg.H, cfg.L, w.tab_len
        drone, counters = SM.at(st.drone, (B, A.DF), np.float64), SM.at(st.counters, (B, A.CF), np.int32)
        seen, last = SM.at(w.seen, (B, W, H), np.int32), SM.at(w.last_call, (B,), np.int32)
        refreshed, obs = SM.at(w.refreshed, (B,), np.int32), SM.at(w.obs, (B, L, L), np.float32)
        tab = SM.at(w.tab, (2, n), np.float64)
        self.seen_updates += 1
        for e in range(B):
            out = SN.update(seen[e], last[e], counters[e, A.C_STEPS], drone[e], cfg, view_range, tab)
            if out is not None:
                last[e], refreshed[e], obs[e] = out


class SeenOracleBackend(_Seen, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+seen'


class SeenTurnBackend(_Seen, AB.TurnPrimitiveBackend):
    name = AB.TurnPrimitiveBackend.name + '+seen'


class SeenTurnJerkBackend(_Seen, AB.TurnJerkBackend):
    name = AB.TurnJerkBackend.name + '+seen'


class SeenJerkBackend(_Seen, LiveJerkBackend):
    name = LiveJerkBackend.name + '+seen'


def env_of(params, B, backend=None, **kw):
    """VecDrone2DEnv of `params` (host-built worlds unless `worlds` says otherwise) with the caller's gaze on a fresh backend, attached"""
    from drone2d_amd import vec_env
    from drone2d_amd.params import with_defaults
    backend = backend or SeenOracleBackend()
    backend.seen_view_range = with_defaults(params).drone_view_range
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', params.planner)
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, **kw)
    return backend.attach(env) if hasattr(backend, 'attach') else env
