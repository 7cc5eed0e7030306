"""Host side of the step path's gaze decision on the device (include/d2d_gaze.h): the table the library takes as an input and the
per-batch state it works on.

`policy.plan(policy, env.info)` of the reference's episode loop (experiment.py:69) runs before every step, on what the previous step
left.  For LookAhead and Owl that is one launch of libd2d_gaze.so over the batch's own buffers; the Owl policy's state (its 36
direction scores, the decision it holds and for how many more calls) lives here, one record per env, in the layout include/d2d.h
defines for the Owl stage, and the table of Owl's constants is the one `device_plugins.owl_table` builds with the reference's own
expressions.
"""
from . import _abi as A

KINDS = {'LookAhead': A.GAZE_K_LOOKAHEAD, 'Owl': A.GAZE_K_OWL}


class GazeState:
    """Table, per-env Owl state and the ctypes d2d_gaze_call over them and over a BatchState."""

    def __init__(self, params, cfg, device, kind):
        import torch
        if kind not in KINDS:
            raise ValueError(f'gaze {kind!r}: the step path decides {sorted(KINDS)} on the device')
        self.cfg, self.device, self.kind = cfg, torch.device(device), kind
        if cfg.N > A.GAZE_MAX_N:
            raise ValueError(f'gaze {kind!r} on the device: {cfg.N} agents per env, at most {A.GAZE_MAX_N}')
        self.owl_tab = self.owl_state = None
        if kind == 'Owl':
            from .device_plugins import owl_table
            self.tab_np = owl_table(params)
            self.owl_tab = torch.from_numpy(self.tab_np).to(self.device)
            self.owl_state = torch.zeros((cfg.B, A.OWL_STATE_F), dtype=torch.float64, device=self.device)
        self.scalars = dict(B=cfg.B, N=cfg.N, kind=KINDS[kind], reserved=0, dt=float(params.dt),
                            yaw_rate_max=float(params.drone_max_yaw_speed))

    def call(self, state, skip_done=True):
        """the d2d_gaze_call that decides for the envs of BatchState `state`; `skip_done`: finished envs are left untouched"""
        c = A.GazeCall()
        for k, v in self.scalars.items():
            setattr(c, k, v)
        for k in ('drone', 'target', 'active', 'kf', 'action'):
            t = state.t.get(k)
            setattr(c, k, t.data_ptr() if t is not None and t.numel() else None)
        c.flags = state.t['flags'].data_ptr() if skip_done and state.t['flags'].numel() else None
        if self.cfg.N == 0:
            c.active = c.kf = None
        if self.owl_state is not None:
            c.owl_state = self.owl_state.data_ptr() if self.owl_state.numel() else None
            c.owl_tab = self.owl_tab.data_ptr()
        return c
