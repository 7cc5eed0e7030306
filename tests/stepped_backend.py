"""Test-side backend for the step path's episode loop with the Primitive plugins without a GPU (VecDrone2DEnv.policy_step /
run_episodes, runner.SteppedExperimentBatch with planner 'Primitive' under RVO): the CPU oracle for every stage of include/d2d.h, its
Oxford gaze stage and its Primitive plan stage included, plus the host RVO build of tests/rvo_backend.py.  The four launches that
leave finished envs alone (include/d2d_stepped.h, include/d2d_rvo_live.h) are the unmasked call followed by putting back everything
of a finished env that the call may have written.  Test infrastructure: the product package never imports this.

The entry points take pointers, so the backend has to be told which env's tensors stand behind them: one backend per env,
`attach(env)` after the env is built (primitive_rvo_cases does it for every env it makes)."""
from rvo_backend import OracleRvoBackend

PLAN_OUT = ('plan_ok', 'wp_valid', 'wp')


class SteppedOracleBackend(OracleRvoBackend):
    name = 'oracle+rvo_host+live'
    supports_stepped_plugins = True
    supports_rvo_live = True
    env = None

    def attach(self, env):
        self.env = env
        return env

    def _done(self):
        return self.env.state.flags[:, self.A.F_DONE].bool()

    def _kept(self, state_names):
        """(tensor, copy) of every per-env buffer a plugin stage may write"""
        env = self.env
        ts = [env.state.t[n] for n in state_names] + [t for k, t in env.plugins.t.items() if k != 'launch_args']
        return [(t, t.clone()) for t in ts]

    @staticmethod
    def _put_back(kept, done):
        for t, old in kept:
            t[done] = old[done]

    def gaze_stage_live(self, cfg, st, plan):
        kept, done = self._kept(('action',)), self._done()
        self.gaze_stage(cfg, st, plan)
        self._put_back(kept, done)

    def plan_stage_live(self, cfg, st, plan):
        kept, done = self._kept(PLAN_OUT), self._done()
        self.plan_stage(cfg, st, plan)
        self._put_back(kept, done)

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
