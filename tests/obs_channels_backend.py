"""Test-side backends for swept_obs, seen_obs and scan_obs switched on together without a GPU: the launch mixins of
tests/swept_backend.py, tests/seen_backend.py and tests/scan_backend.py combined over the bases the per-channel files use one at a
time.  Nothing is restated here: a launch is the model its own file gives it.  `log` (a list, or None) receives the name of every
launch of a step in the order the env queued it, for the launch-order test.  Test infrastructure: the product package never imports
this."""
import action_stream_backend as AB
from jerk_live_backend import LiveJerkBackend
from scan_backend import _Scan
from seen_backend import _Seen
from stepped_backend import SteppedOracleBackend
from swept_backend import SweptJerkBackend, _Swept

LOGGED = ('gaze_stage_live', 'rvo_velocity_live', 'rvo_agents_step_live', 'rvo_velocity', 'rvo_agents_step', 'run_stages', 'perceive', 'act',
          'step', 'closed_loop', 'plan_stage', 'plan_stage_live', 'jerk_plan', 'jerk_plan_live', 'gaze_act', 'swept_mark', 'swept_crop',
          'seen_update', 'scan_update')


def _label(name, args):
    """d2d_run_stages is the perceive launch, the act launch or the whole step by its stage bits; the masked launches are the launch"""
    from drone2d_amd import _abi as A
    if name == 'run_stages':
        bits = int(args[2])
        return 'step' if bits & A.ST_RAYCAST and bits & A.ST_CONTROL else ('perceive' if bits & A.ST_RAYCAST else 'act')
    return {'plan_stage_live': 'plan', 'plan_stage': 'plan', 'jerk_plan_live': 'plan', 'jerk_plan': 'plan'}.get(name, name)


class _Logged:
    """every launch named in LOGGED that the env itself queues appends its label to `log` where a test has set one.  (The model
    backends nest launches -- a masked launch calls the unmasked one and puts the finished envs back -- and what a launch calls is
    not the env's)"""
    log = None
    _depth = 0

    def __getattribute__(self, name):
        value = object.__getattribute__(self, name)
        if name in LOGGED and callable(value) and object.__getattribute__(self, 'log') is not None:
            def logged(*a, _f=value, _n=name, **k):
                if self._depth == 0:
                    self.log.append(_label(_n, a))
                self._depth += 1
                try:
                    return _f(*a, **k)
                finally:
                    self._depth -= 1
            return logged
        return value


class ChannelsOracleBackend(_Logged, _Swept, _Seen, _Scan, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+swept+seen+scan'


class ChannelsTurnBackend(_Logged, _Swept, _Seen, _Scan, AB.TurnPrimitiveBackend):
    name = AB.TurnPrimitiveBackend.name + '+swept+seen+scan'


class _SweptZero:
    """Jerk_Primitive: the swept channel is a resident zero tensor and neither launch is ever queued (tests/swept_backend.py)"""
    supports_swept_obs = True
    swept_mark = swept_crop = SweptJerkBackend.swept_mark


class ChannelsJerkBackend(_Logged, _SweptZero, _Seen, _Scan, LiveJerkBackend):
    name = LiveJerkBackend.name + '+swept+seen+scan'


class ChannelsTurnJerkBackend(_Logged, _SweptZero, _Seen, _Scan, AB.TurnJerkBackend):
    name = AB.TurnJerkBackend.name + '+swept+seen+scan'


def stream_backend_for(params):
    """the combined backend an action stream / episode stream of `params` runs on"""
    return (ChannelsTurnJerkBackend if params.planner == 'Jerk_Primitive' else ChannelsTurnBackend)().of(params)


def backend_for(params):
    """the combined backend of an env with host-built worlds"""
    return (ChannelsJerkBackend if params.planner == 'Jerk_Primitive' else ChannelsOracleBackend)()


def env_of(params, B, backend=None, **kw):
    """VecDrone2DEnv of `params` (host-built worlds unless `worlds` says otherwise) with the caller's gaze on a fresh combined
    backend, attached; the channels are the keywords"""
    from drone2d_amd import vec_env
    from drone2d_amd.params import with_defaults
    backend = backend or backend_for(params)
    backend.seen_view_range = with_defaults(params).drone_view_range
    kw.setdefault('gaze', 'external')
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', params.planner)
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, **kw)
    return backend.attach(env) if hasattr(backend, 'attach') else env


def stream_env_of(params, slots, **kw):
    """... with device worlds on the combined turn backend: what action_stream() and stream_episodes() need"""
    return AB.env_of(params, slots, backend=stream_backend_for(params), **kw)
