"""The device noise stream (d2d_state.rng) against the oracle driven with host draws: the case table and the oracle side of
tests/test_gpu_device_noise.py (test infrastructure, like closed_loop_cases.py).

The oracle has no stream of its own: it takes the draws as an input.  Which agents a step draws for is decided by that step's own
raycast, so the oracle side runs every step twice -- once dry (zero noise) to learn `hit`, which no draw can change, then, from
the saved state, with np.random.randn(2) drawn for every hit agent in agent order from a RandomState restored to the env's
initial stream: what env.py's _perceive does between the raycast and the trackers, for every launch path's own step."""
import numpy as np
import torch

from rng_host import RNG_NPAIR, RNG_NREGEN, assert_state_is, numpy_stream

# var_cam = 2 keeps every configuration off the specialised kernels (their sigma is the literal 0): the generic step kernel,
# k_closed<0> / <4> and the per-stage loops.  A wide, deep view and many large agents: several agents in view at once, so that a
# 50-step episode uses up the 106 attempts the key has left after world construction.
_VIEW = dict(var_cam=2, drone_view_range=160, drone_view_depth=120, agent_radius=14, agent_max_speed=30)
_WORLD = dict(map_size=[600, 450], init_pos=[300, 220], target_list=[[520, 380]])


def _row(name, path, kind, on_done, B, T, chunks, layout='rowmajor', planner='Primitive', gaze='Oxford', **kw):
    return dict(name=name, path=path, kind=kind, on_done=on_done, B=B, T=T, chunks=chunks, layout=layout, planner=planner, gaze=gaze,
                kw=dict(_VIEW, **kw))


CASES = [
    # ---- the step kernel: fused, queued back to back, and cut between the raycast and the trackers
    _row('step', None, 'step', 'continue', 4, 100, [1], planner='NoMove', gaze=None, agent_number=16, map_id=501, max_flight_time=30),
    _row('rollout', None, 'rollout', 'continue', 5, 100, [7, 1, 13], planner='NoMove', gaze=None, agent_number=24, map_id=502,
         max_flight_time=30, **_WORLD),
    _row('split', None, 'split', 'continue', 3, 90, [1], planner='NoMove', gaze=None, layout='tiled', agent_number=12, map_id=503,
         max_flight_time=30, map_size=[530, 470], init_pos=[260, 230]),
    # ---- the per-stage closed loops
    _row('stage_nomove-freeze', 'per_stage_nomove', 'closed', 'freeze', 5, 100, [7, 3], planner='NoMove', gaze='Rotating',
         agent_number=24, map_id=511, max_flight_time=9, agent_max_speed=40),
    _row('stage_nomove-reset', 'per_stage_nomove', 'closed', 'reset', 3, 120, [9, 4], planner='NoMove', gaze='Oxford',
         agent_number=24, map_id=512, max_flight_time=5, **_WORLD),
    _row('stage_primitive-reset', 'per_stage_primitive', 'closed', 'reset', 3, 120, [5, 8], agent_number=24, map_id=513,
         max_flight_time=5, **_WORLD),
    _row('stage_primitive-continue', 'per_stage_primitive', 'closed', 'continue', 4, 80, [1, 12], gaze='NoControl', agent_number=12,
         map_id=514, max_flight_time=4, **_WORLD),
    # ---- the persistent kernels
    _row('closed0-continue', 'k_closed<0>', 'closed', 'continue', 6, 100, [7, 13], agent_number=20, map_id=521, max_flight_time=6,
         **_WORLD),
    _row('closed0-reset', 'k_closed<0>', 'closed', 'reset', 3, 120, [11, 1, 6], agent_number=20, map_id=526, max_flight_time=5,
         **_WORLD),
    _row('closed0-freeze', 'k_closed<0>', 'closed', 'freeze', 5, 100, [9], gaze='Rotating', agent_number=24, map_id=523,
         max_flight_time=7, **_WORLD),
    _row('closed4-reset', 'k_closed<4>', 'closed', 'reset', 3, 120, [6, 9], layout='tiled', agent_number=24, map_id=531,
         max_flight_time=5, map_size=[530, 470], init_pos=[450, 60], target_list=[[80, 400]]),
    _row('closed4-freeze', 'k_closed<4>', 'closed', 'freeze', 4, 100, [1, 14], layout='tiled', gaze='NoControl', agent_number=20,
         map_id=532, max_flight_time=6, map_size=[470, 530], init_pos=[60, 60], target_list=[[400, 470]]),
]


def case_id(c):
    return c['name']


def params_of(pkg, c):
    return pkg.Params(planner=c['planner'], gaze_method=c['gaze'] or 'NoControl', **c['kw'])


def make_env(pkg, backend, c, worlds, device_side):
    from drone2d_amd import vec_env
    kw = dict(backend=backend, planner=c['planner'], worlds=worlds)
    if c['kind'] == 'closed':
        kw.update(device_plugins=True, gaze=c['gaze'])
    if device_side:
        kw.update(grid_layout=c['layout'])
    env = vec_env.VecDrone2DEnv(params_of(pkg, c), c['B'], **kw)
    if c['path'] == 'per_stage_primitive' and device_side:
        env._plan.launch_args = None
    return env


def mode_of(c):
    return {'continue': {}, 'reset': dict(auto_reset=True), 'freeze': dict(freeze_done=True)}[c['on_done']]


class OracleWithHostDraws:
    """The oracle env of a row, stepped one step at a time with numpy's draws (module docstring)"""

    def __init__(self, pkg, oracle, c, worlds):
        self.A, self.c = pkg._abi, c
        self.env = make_env(pkg, oracle, c, worlds, device_side=False)
        assert not self.env.device_noise                       # the oracle takes its draws as an input
        B, N = c['B'], self.env.N
        self.init = [np.asarray(w['rng'], dtype=np.uint32).copy() for w in worlds]
        self.rs = [numpy_stream(s) for s in self.init]
        self.pairs = np.zeros(B, dtype=np.int64)               # pairs drawn since the stream was (re)seeded
        self.draws = np.zeros((B, N, 2))                       # what d2d_state.rng_draws has to hold
        self.seen = dict(none=False, many=False, done=False)
        self.episodes = [[[]] for _ in range(B)]               # per env: per episode: a record of every step

    def _tensors(self):
        t = dict(('s.' + k, v) for k, v in self.env.state.t.items())
        if self.env.plugins is not None:
            t.update(('p.' + k, v) for k, v in self.env.plugins.t.items())
        return t

    def _run(self, action):
        if self.c['kind'] == 'closed':
            self.env.closed_loop(1, **mode_of(self.c))
        else:
            self.env.step(action)

    def step(self, action=None):
        env, A, c = self.env, self.A, self.c
        B, N = c['B'], env.N
        done = env.state.flags[:, A.F_DONE].numpy() != 0
        closed = c['kind'] == 'closed'
        frozen = done & (closed and c['on_done'] == 'freeze')
        restart = done & (closed and c['on_done'] == 'reset')
        saved = {k: v.clone() for k, v in self._tensors().items()}
        env.set_noise(np.zeros((B, N, 2)))
        self._run(action)                                      # dry: which agents does this step's raycast hit?
        hit = env.state.hit.numpy() != 0
        for k, v in self._tensors().items():
            v.copy_(saved[k])
        for e in range(B):
            if frozen[e]:
                continue                                       # the env does not step: its stream and its draws stay
            if restart[e]:                                     # reset() re-seeds, envs/drone_v2.py:259-261
                self.rs[e], self.pairs[e] = numpy_stream(self.init[e]), 0
                self.episodes[e].append([])
            self.draws[e] = 0.0
            for k in np.flatnonzero(hit[e]):
                self.draws[e, k] = self.rs[e].randn(2)
            m = int(hit[e].sum())
            self.pairs[e] += m
            self.seen['none'] |= m == 0
            self.seen['many'] |= m >= 2
        env.set_noise(self.draws)
        self._run(action)
        assert np.array_equal(env.state.hit.numpy() != 0, hit)
        self.seen['done'] |= bool(env.state.flags[:, A.F_DONE].any())
        for e in range(B):
            if not frozen[e]:
                self.episodes[e][-1].append((self.draws[e].tobytes(), env.state.drone[e].numpy().tobytes(),
                                             env.state.kf[e].numpy().tobytes(), self.rs[e].get_state()[2]))

    def check_stream(self, dev, tag):
        """The device's streams and draws against numpy's: key, position, pairs and regenerations counted, the draws of the step"""
        rng = dev.state.rng.cpu().numpy().view(np.uint32)
        got = dev.state.rng_draws.cpu().numpy()
        assert got.tobytes() == self.draws.tobytes(), f'{tag}: rng_draws differ at {np.argwhere(got != self.draws)[:5].tolist()}'
        for e in range(self.c['B']):
            assert_state_is(rng[e], self.rs[e], f'{tag}: env {e}')
            assert int(rng[e, RNG_NPAIR]) == int(self.pairs[e]) & 0xffffffff, f'{tag}: env {e} pairs'
        return int(rng[:, RNG_NREGEN].max())


def assert_same_state(dev, ref, tag, plugins, skip=()):
    """Every field of the env state (the grids in the reference's indexing) and of the plugin state but the search scratch"""
    dev.sync()
    for name, b in ref.state.t.items():
        if name in ('rng', 'rng_draws') or name in skip:
            continue                                           # (rng: the oracle has none -- OracleWithHostDraws.check_stream)
        a = dev.state.logical(name).cpu()
        assert torch.equal(a, b), f'{tag}: field {name} differs at {(a != b).nonzero()[:5].tolist()}'
    if plugins:
        hd = ref.plugins.t['traj_hdr']
        for name in ('traj_hdr', 'trk_radius', 'trk_prev', 'seen_step'):
            a, b = dev.plugins.t[name].cpu(), ref.plugins.t[name]
            assert torch.equal(a, b), f'{tag}: plugin field {name} differs at {(a != b).nonzero()[:5].tolist()}'
        ta, tb = dev.plugins.t['traj'].cpu(), ref.plugins.t['traj']
        for e in range(ref.num_envs):
            h, n = int(hd[e, 0]), int(hd[e, 1])
            assert torch.equal(ta[e, h:n], tb[e, h:n]), f'{tag}: trajectory of env {e}'
