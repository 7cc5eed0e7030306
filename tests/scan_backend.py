"""Test-side backend for scan_obs=True without a GPU: the launch of include/d2d_scan.h done by tests/scan_model.py on the host memory
behind the structs' pointers, mixed into the oracle backends of the other test modules.  The CPU stand-in the other libraries'
*_backend.py files are.  Test infrastructure: the product package never imports this."""
import numpy as np

import action_stream_backend as AB
import scan_model as SN
import stream_model as SM
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend


def grid_bytes(cfg):
    return ((cfg.W + 15) // 16) * ((cfg.H + 15) // 16) * 256 if cfg.grid_tile else cfg.W * cfg.H


def views(cfg, st, w):
    """numpy views of everything d2d_scan_update reads and writes, behind host pointers"""
    B, N, R, hw = cfg.B, cfg.N, cfg.R, w.hit_words
    return dict(agents=SM.at(st.agents, (B, A.AF, N), np.float64), counters=SM.at(st.counters, (B, A.CF), np.int32),
                gt=SM.at(st.gt, (B, grid_bytes(cfg)), np.uint8), pose=SM.at(w.pose, (B, A.DF), np.float64),
                end=SM.at(w.end, (B, R, 2), np.float64), kind=SM.at(w.kind, (B, R), np.uint8), hit=SM.at(w.hit, (B, R, hw), np.uint32),
                obs=SM.at(w.obs, (B, 2, R), np.float32), last_step=SM.at(w.last_step, (B,), np.int32))


def model_update(cfg, st, w):
    """d2d_scan_update by the model"""
    v = views(cfg, st, w)
    for e in range(cfg.B):
        steps = v['counters'][e, A.C_STEPS]
        out = SN.update(v['last_step'][e], steps, v['pose'][e], v['agents'][e], v['gt'][e], cfg, w.hit_words)
        if out is not None:
            v['end'][e], v['kind'][e], v['hit'][e], v['obs'][e] = out
            v['last_step'][e] = steps


class _Scan:
    supports_scan_obs = True
    scan_updates = 0

    def scan_update(self, cfg, st, w):
        self.scan_updates += 1
        model_update(cfg, st, w)


class ScanOracleBackend(_Scan, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+scan'


class ScanTurnBackend(_Scan, AB.TurnPrimitiveBackend):
    name = AB.TurnPrimitiveBackend.name + '+scan'


class ScanTurnJerkBackend(_Scan, AB.TurnJerkBackend):
    name = AB.TurnJerkBackend.name + '+scan'


class ScanJerkBackend(_Scan, LiveJerkBackend):
    name = LiveJerkBackend.name + '+scan'


def env_of(params, B, backend=None, **kw):
    """VecDrone2DEnv of `params` (host-built worlds unless `worlds` says otherwise) with the caller's gaze on a fresh backend, attached"""
    from drone2d_amd import vec_env
    backend = backend or ScanOracleBackend()
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', params.planner)
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, **kw)
    return backend.attach(env) if hasattr(backend, 'attach') else env
