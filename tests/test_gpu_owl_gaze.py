"""Owl as a device gaze stage (run with -m gpu): the golden Owl episodes stepped and in one persistent call, ExperimentBatch('Owl'),
every launch path of d2d_closed_loop under continue / reset / freeze, a randomised soak and a 4096-env property run.

The oracle has no Owl stage.  The checker is the reference's recorded episodes (tests/golden) plus the scalar model of
tests/owl_model.py: the oracle steps the same batch one step at a time with gaze='external' and takes its actions from one model
per env, fed the oracle's own state; the device must reproduce every state field, every action and its Owl state bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import closed_loop_cases as CL
import owl_model as OM
from replay import load
from test_gpu_closed_loop_paths import SCRATCH, _mode, _snapshot
from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import _worlds
from test_owl_gaze_cpu import EPISODES, episode_id

pytestmark = pytest.mark.gpu


def _row(r):
    return np.array([float(v) for v in r[12:]], dtype=np.float64)


def _batch(pkg, hip, fixture, case, B):
    from drone2d_amd import runner
    fx = load(fixture)
    kw = json.loads(str(fx[f'r{case}_cfg']))
    p = pkg.Params(debug=True, **kw)
    p.render = False
    eb = runner.ExperimentBatch(p, B, device=hip.device, backend=hip)
    assert eb.env._plan.gaze == pkg._abi.GAZE_OWL and eb.env._plan.owl_tab and eb.env._plan.owl_state
    return fx, kw, eb


def _owl_state(env):
    return env.plugins.t['owl_state'].cpu().numpy()


@pytest.mark.parametrize('ep', EPISODES, ids=episode_id)
def test_reference_episodes_as_device_closed_loops(pkg, hip, ep):
    """Every golden Owl episode as a device closed loop, one step per call: every action's bits are the reference's, the Owl state
    after every call is the model's (and the scores the reference's U_list where the fixture holds it), the CSV row is the
    reference's.  Then the same episode in ONE closed_loop call on the persistent kernel: the final state equals the stepped run's."""
    A = pkg._abi
    fx, _, eb = _batch(pkg, hip, ep[0], ep[1], 1)
    env, case = eb.env, ep[1]
    want = fx[f'r{case}_actions']
    scores = fx[f'r{case}_scores'] if f'r{case}_scores' in fx.files else None
    model = OM.OwlModel.from_params(env.params)
    acts, decisions = [], 0
    while not acts or not bool(env.state.flags[0, A.F_DONE]):
        t, args = len(acts), OM.inputs_of(OM.host_state(env), 0)
        assert t < len(want), f'{ep}: the episode outlives the reference ({len(want)} steps)'
        a_model = model.plan(*args)
        decisions += model.decided
        env.closed_loop(1, freeze_done=True)
        a = float(env.state.action[0])
        acts.append(a)
        tag = f'{ep} step {t + 1}'
        assert np.float64(a).view(np.int64) == want[t].view(np.int64), f'{tag}: action {a!r}, reference {float(want[t])!r}'
        assert a == a_model, f'{tag}: action {a!r}, model {a_model!r}'
        st = _owl_state(env)[0]
        assert np.array_equal(st, model.state()), f'{tag}: owl_state {st.tolist()} vs model {model.state().tolist()}'
        assert np.array_equal(env.plugins.owl_scores(0), st[:A.OWL_NDIR])
        if scores is not None:
            assert np.array_equal(st[:A.OWL_NDIR], scores[t]), f'{tag}: scores vs the reference U_list'
    assert len(acts) == len(want) and decisions >= len(want) // 8
    got_row, want_row = _row(eb.rows()[0]), fx[f'r{case}_row']
    print(f'{ep}: {len(acts)} steps, {decisions} decisions, row {got_row.tolist()}')
    assert np.allclose(got_row, want_row, rtol=0, atol=1e-9, equal_nan=True), (got_row, want_row)
    # one call, persistent kernel
    _, _, eb2 = _batch(pkg, hip, ep[0], ep[1], 1)
    assert CL.closed_loop_path(eb2.env.cfg, eb2.env._plan).startswith('k_closed<')
    eb2.env.closed_loop(len(want), freeze_done=True)
    a, b = _snapshot(env)[0], _snapshot(eb2.env)[0]
    for k in a:
        if k[2:] not in SCRATCH:
            assert torch.equal(a[k], b[k]), f'{ep}: {k} of the one-call run differs from the stepped run'


def test_experiment_batch_owl(pkg, hip):
    """ExperimentBatch with Owl on 5 envs: row 0 is the reference's row, rows 1-4 equal stand-alone Experiment runs (the package's
    host policy gaze.Owl on the env facade)."""
    from drone2d_amd import runner
    fx, kw, eb = _batch(pkg, hip, 'host_gaze_rows', 3, 5)
    rows = eb.run()
    assert all(int(d) for d in eb.env.state.flags[:, pkg._abi.F_DONE].cpu())
    assert np.allclose(_row(rows[0]), fx['r3_row'], rtol=0, atol=1e-9, equal_nan=True), _row(rows[0])
    for e in range(1, 5):
        q = pkg.Params(debug=True, **dict(kw, map_id=kw['map_id'] + e))
        q.render = False
        want = runner.Experiment(q, device=hip.device, backend=hip).run()
        assert rows[e][3] == want[3] and np.allclose(_row(rows[e]), _row(want), rtol=0, atol=1e-9, equal_nan=True), e


# ---------------------------------------------------------------------------------------------------------------------------
# device vs oracle + model
# ---------------------------------------------------------------------------------------------------------------------------
class ModelDriver:
    """One OwlModel per env of an oracle batch stepped with gaze='external'"""

    def __init__(self, ref, on_done):
        self.ref, self.on_done = ref, on_done
        self.models = [OM.OwlModel.from_params(ref.params) for _ in range(ref.num_envs)]
        self.ended = self.restarted = 0
        self.decisions = self.nan_decisions = self.with_trackers = 0

    def step(self, pkg, mode):
        A, ref = pkg._abi, self.ref
        done = ref.state.flags[:, A.F_DONE].numpy() != 0
        if self.on_done == 'reset' and done.any():            # the device resets a finished env at the start of its next step
            ref.reset(torch.from_numpy(done.astype(np.uint8)))
            for e in np.flatnonzero(done):
                self.models[e] = OM.OwlModel.from_params(ref.params)          # a fresh policy per episode (experiment.py:31-34)
                self.restarted += 1
            done[:] = False
        envs = np.flatnonzero(~done) if self.on_done == 'freeze' else np.arange(ref.num_envs)   # a frozen env keeps its action
        hs = OM.host_state(ref)
        for e in envs:
            m = self.models[e]
            ref.state.action[e] = m.plan(*OM.inputs_of(hs, e))
            if m.decided:
                self.decisions += 1
                self.nan_decisions += bool(np.isnan(m.costs).all())
                self.with_trackers += bool(hs['active'][e].any())
        ref.closed_loop(1, **mode)
        self.ended += int(bool((ref.state.flags[:, A.F_DONE] != 0).any()))        # steps that left a finished env behind

    def owl_state(self):
        return np.stack([m.state() for m in self.models])


def _assert_same_owl(dev, drv, tag):
    _assert_same(dev, drv.ref, tag)
    got, want = _owl_state(dev), drv.owl_state()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{tag}: owl_state differs at {bad[:5].tolist()} ({len(bad)} elements): '
                             f'{[(got[tuple(i)], want[tuple(i)]) for i in bad[:5]]}')


def _owl_row(path, on_done, B, T, chunks, layout='rowmajor', noise=False, **kw):
    return dict(path=path, gaze='Owl', policy='Owl', on_done=on_done, B=B, T=T, chunks=chunks, layout=layout, noise=noise,
                zero_call=False, null_box=False, kw=kw)


_PATH_SETS = {      # the parameter sets of closed_loop_cases' rows, one per launch path
    'k_closed<1>': dict(agent_number=12, **CL._NEAR, **CL._FAST),
    'k_closed<2>': dict(agent_number=30, agent_radius=10, agent_max_speed=60, **CL._NEAR),
    'k_closed<3>': dict(agent_number=48, agent_radius=8, agent_max_speed=60, **CL._NEAR),
    'k_closed<0>': dict(agent_number=20, agent_radius=12, agent_max_speed=30, map_size=[600, 450], init_pos=[300, 220],
                        target_list=[[520, 380]], **CL._OTHER),
    'k_closed<4>': dict(agent_number=14, agent_radius=12, agent_max_speed=40, map_size=[530, 470], init_pos=[450, 60],
                        target_list=[[80, 400]], **CL._OTHER),
    'per_stage_nomove': dict(agent_number=20, agent_radius=15, agent_max_speed=60, init_pos=[250, 250], max_flight_time=6),
    'per_stage_primitive': dict(agent_number=10, **CL._NEAR, **CL._FAST),
}
_CHUNKS = {'continue': [7], 'reset': [1, 9], 'freeze': [5, 12, 3]}
OWL_CASES = [_owl_row(path, on_done, 3, 100, _CHUNKS[on_done], layout='tiled' if path == 'k_closed<4>' else 'rowmajor',
                      noise=(on_done == 'continue' and path in ('k_closed<0>', 'per_stage_primitive')),
                      map_id=500 + 10 * i + j, **dict(kw, **(dict(var_cam=2) if on_done == 'continue' and path in
                                                             ('k_closed<0>', 'per_stage_primitive') else {})))
             for i, (path, kw) in enumerate(_PATH_SETS.items()) for j, on_done in enumerate(CL.ON_DONE)]
assert set(c['path'] for c in OWL_CASES) == set(CL.PATHS) and len(OWL_CASES) == len(CL.PATHS) * len(CL.ON_DONE)


def owl_envs(pkg, hip, oracle, c):
    """The row's oracle env (gaze='external') and, with a GPU backend, the device env on the same worlds"""
    from drone2d_amd import vec_env
    p, planner = CL.params_of(pkg, c), CL.planner_of(c)
    ref = vec_env.VecDrone2DEnv(p, c['B'], backend=oracle, planner=planner, device_plugins=True, gaze='external')
    dev = None
    if hip is not None:
        dev = vec_env.VecDrone2DEnv(p, c['B'], backend=hip, planner=planner, device_plugins=True, gaze='Owl', worlds=_worlds(ref),
                                    grid_layout=c['layout'])
        CL.adjust_plan(c, dev._plan)
    if c['noise']:
        noise = np.random.RandomState(c['kw']['map_id']).standard_normal((CL.NOISE_ROWS, c['B'], ref.N, 2))
        for env in (dev, ref):
            if env is not None:
                env.set_noise(noise)
    return dev, ref


@pytest.mark.parametrize('case', OWL_CASES, ids=CL.case_id)
def test_closed_loop_path_with_owl_matches_oracle_and_model(pkg, hip, oracle, case):
    c, name = case, CL.case_id(case)
    dev, ref = owl_envs(pkg, hip, oracle, c)
    assert CL.closed_loop_path(dev.cfg, dev._plan) == c['path'], name
    drv = ModelDriver(ref, c['on_done'])
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        t = 0
        for n in CL.chunk_sizes(c):
            dev.closed_loop(n, **_mode(c))
            for _ in range(n):
                drv.step(pkg, _mode(c))
            t += n
            _assert_same_owl(dev, drv, f'{name} after step {t}')
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    print(f'{name}: {drv.decisions} decisions, {drv.nan_decisions} all-NaN, {drv.with_trackers} with an active tracker, '
          f'{drv.ended} ended, {drv.restarted} restarted')
    assert drv.ended > 0, f'{name}: no episode ended'
    assert drv.decisions >= c['B']                       # every env decides at its first call (a frozen env decides no more)
    if c['on_done'] == 'reset':
        assert drv.restarted > 0, f'{name}: no episode restarted'
        dev.reset()                                      # d2d_plan_reset: a fresh policy is all zero
        assert not _owl_state(dev).any()


def _soak_cfg(seed):
    rng = np.random.RandomState(7000 + seed)
    size = [[500, 500], [600, 450], [700, 400], [800, 600], [450, 650]][int(rng.randint(5))]
    kw = dict(agent_number=int(rng.randint(2, 41)), agent_radius=int(rng.choice([5, 8, 10, 12, 15])),
              agent_max_speed=int(rng.choice([10, 20, 30, 40, 60])), drone_max_speed=int(rng.choice([20, 30, 40, 50, 60])),
              map_id=int(rng.randint(0, 10000)), drone_view_range=int(rng.choice([60, 90, 120, 360])),
              drone_view_depth=int(rng.choice([60, 80, 100])), drone_max_yaw_speed=int(rng.choice([40, 80, 120])),
              map_size=size, init_pos=[int(rng.randint(60, size[0] - 60)), int(rng.randint(60, size[1] - 60))],
              target_list=[[int(rng.randint(40, size[0] - 40)), int(rng.randint(40, size[1] - 40))]],
              dt=float(rng.choice([0.1, 0.2])))
    if rng.rand() < 0.3:
        kw['max_flight_time'] = 6
    if rng.rand() < 0.25:
        kw['pillar_number'] = int(rng.randint(1, 6))
    return kw, dict(planner='NoMove' if seed % 9 == 4 else 'Primitive', B=int(rng.choice([3, 4, 6])),
                    chunk=int(rng.choice([1, 4, 8, 15])), on_done=('reset', 'freeze', 'continue')[seed % 3])


@pytest.mark.parametrize('seed', list(range(int(os.environ.get('D2D_OWL_SEEDS', '32')))))
def test_random_owl_gaze_matches_oracle_and_model(pkg, hip, oracle, seed):
    """Device closed loop with Owl for 120 steps over random agent counts, speeds, radii, fields of view, view depths, map sizes and
    dt in {0.1, 0.2} vs the oracle stepping the same batch with the model's actions: the whole env and plugin state and the Owl
    state bit for bit after every call."""
    kw, r = _soak_cfg(seed)
    c = dict(policy='Owl', path='per_stage_nomove' if r['planner'] == 'NoMove' else '', B=r['B'], layout='rowmajor', noise=False,
             null_box=False, on_done=r['on_done'], kw=kw)
    dev, ref = owl_envs(pkg, hip, oracle, c)
    drv = ModelDriver(ref, r['on_done'])
    assert drv.models[0].hold == OM.hold_calls(kw['dt']) >= 0
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        for t0 in range(0, 120, r['chunk']):
            n = min(r['chunk'], 120 - t0)
            dev.closed_loop(n, **_mode(c))
            for _ in range(n):
                drv.step(pkg, _mode(c))
            _assert_same_owl(dev, drv, f'seed {seed} {r} {kw} after step {t0 + n}')
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    assert drv.decisions >= r['B']                       # every env decides at its first call


def test_owl_full_size_property_run(pkg, hip):
    """4096 envs x 10 agents (the README configuration), 240 steps with auto reset: every action is one of the table's 20 values,
    the countdown stays in [0, hold], the scores stay in [0, 1]."""
    from drone2d_amd import vec_env
    A = pkg._abi
    p = pkg.Params(planner='Primitive', gaze_method='Owl', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
                   map_id=1)
    B = 4096
    env = vec_env.VecDrone2DEnv(p, B, backend=hip, planner='Primitive', device_plugins=True, gaze='Owl',
                                worlds=vec_env.build_worlds(p, B, workers=16))
    tab = env.plugins.tables_np['owl_tab']
    allowed, hold = set(tab[A.OWL_T_ACT:A.OWL_T_ACT + A.OWL_NRATE].tolist()), tab[A.OWL_T_HOLD]
    seen = set()
    for n in (1, 7, 40, 64, 128):
        env.closed_loop(n, auto_reset=True)
        st, acts = _owl_state(env), env.state.action.cpu().numpy()
        assert set(acts.tolist()) <= allowed
        seen |= set(acts.tolist())
        left = st[:, A.OWL_S_LEFT]
        assert ((left >= 0) & (left <= hold) & (left == np.floor(left))).all()
        assert set(st[:, A.OWL_S_RATE].tolist()) <= set(tab[:A.OWL_NRATE].tolist())
        assert ((st[:, :A.OWL_NDIR] >= 0) & (st[:, :A.OWL_NDIR] <= 1)).all() and not st[:, 38:].any()
    assert len(seen) >= 9 and bool((env.state.counters[:, A.C_STEPS] < 240).any())      # many rates picked; episodes restarted
