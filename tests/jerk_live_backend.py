"""Test-side backend for whole Jerk_Primitive episodes with every launch leaving finished envs alone, without a GPU
(VecDrone2DEnv.run_episodes(live=...), include/d2d_jerk_live.h): tests/gaze_backend.OracleGazeBackend (the CPU oracle for the stages of
include/d2d.h, the host builds of the planner and of the gaze decision) and tests/rvo_backend.OracleRvoBackend (the host RVO build)
in one class.  d2d_jerk_plan_live is the unmasked call followed by putting back a finished env's seven buffers, and the two launches
of include/d2d_rvo_live.h are made the same way, as tests/stepped_backend.py makes them for the Primitive stages.  `Recording` wraps
any backend and lists the calls it gets.  Test infrastructure: the product package never imports this.

d2d_jerk_plan_live gets the call's pointers, so the backend has to be told which env's tensors stand behind them: one backend per
env, `attach(env)` after the env is built."""
from gaze_backend import OracleGazeBackend
from rvo_backend import OracleRvoBackend

PLAN_STATE = ('plan_ok', 'wp_valid', 'wp')                   # of env.state.t
PLAN_OWN = ('choice', 'stat', 'trk_radius', 'trk_prev')      # of env.jerk.t


class UnmaskedBackend(OracleGazeBackend, OracleRvoBackend):
    """the launches of before include/d2d_jerk_live.h: what run_episodes(live=None) finds on a backend without the masked ones"""
    name = 'oracle+jerk_host+gaze_host+rvo_host'


class LiveJerkBackend(UnmaskedBackend):
    name = 'oracle+jerk_host+gaze_host+rvo_host+live'
    supports_jerk_live = True
    supports_rvo_live = True
    env = None

    def attach(self, env):
        self.env = env
        return env

    def jerk_plan_live(self, call, flags):
        assert flags is not None and flags is self.env.state.flags
        env = self.env
        kept = [(t, t.clone()) for t in [env.state.t[n] for n in PLAN_STATE] + [env.jerk.t[n] for n in PLAN_OWN]]
        done = flags[:, self.A.F_DONE].bool()
        self.jerk_plan(call)
        for t, old in kept:
            t[done] = old[done]

    def rvo_velocity_live(self, agents, vel, pillars, flags, vel_out):
        assert flags is not None
        done = flags[:, self.A.F_DONE].bool()
        self.rvo_velocity(agents, vel, pillars, vel_out)
        vel_out[done] = vel[done]

    def rvo_agents_step_live(self, agents, vel, flags, W_px, H_px, scale, dt):
        assert flags is not None
        done, old = flags[:, self.A.F_DONE].bool(), agents.clone()
        self.rvo_agents_step(agents, vel, W_px, H_px, scale, dt)
        agents[done] = old[done]


LAUNCHES = ('gaze_act', 'rvo_velocity', 'rvo_agents_step', 'rvo_velocity_live', 'rvo_agents_step_live', 'run_stages', 'jerk_plan',
            'jerk_plan_live', 'step', 'perceive', 'act')


class Recording:
    """`inner` with the names of the launches it is asked for kept in `calls` (run_stages with its stage mask)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        got = getattr(self.inner, name)
        if name not in LAUNCHES:
            return got

        def call(*args, **kw):
            self.calls.append((name, args[2]) if name == 'run_stages' else name)
            return got(*args, **kw)
        return call
