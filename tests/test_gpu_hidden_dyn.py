"""The deferred dynamic-grid update of the persistent closed loop (run with -m gpu).  Inside the whole-grid k_closed kernels an env's
dynamic-grid stage runs only on a dyn-visible step (include/d2d.h, d2d_closed_loop; csrc/d2d_hip.hip, dyn_skip): the last of
a launch, every step under D2D_OBS_EVERY_STEP=1 or D2D_DONE_FREEZE, every step of an env whose grid failed the gate (dyn_gate_full).
After a launch every buffer -- gt and dyn_prev first of all -- must hold what the every-step kernel leaves.

For every launch site of the loop two device envs on the same worlds, one of them with D2D_OBS_EVERY_STEP=1: calls of 1, 2 and 3 steps
and one of 40 to 60 under CONTINUE, RESET and FREEZE, compared bit for bit after every call, and both against the oracle.  In every
shape at least one env of the 16 ends its episode inside the longer call (asserted), so under RESET envs restart from the snapshot --
and pass the gate again -- on steps nobody sees.  A short max_flight_time does that for the generic kernel alone: the specialised
kernels are picked only with max_steps == 800 (d2d_plan_spec.h, spec_default_matches), so a shorter one would move the case to
another launch site; there the episodes end by a near target or by fast, large agents, as in tests/test_gpu_hidden_obs.py.
The hand-edited grids of tests/test_hidden_dyn_rule_cpu.py, on which deferring would be wrong, must equal the oracle: the gate sends
those envs down the every-step path."""
import numpy as np
import pytest
import torch

import closed_loop_cases as CL
from test_gpu_hidden_obs import MODES, SHORT, _devices, _same, _snapshot, every_step, ref_call, ref_env
from test_gpu_plugins import _assert_same
from test_gpu_vs_oracle import _worlds
from test_plan_spec_cpu import matches, spec  # noqa: F401  (`spec`: the host build of d2d_plan_spec.h, a fixture)

pytestmark = pytest.mark.gpu

B = 16
# the README's world (bench.py's config 2) with the target 140 px from the start: at 40 px/s an episode lasts some 40 to 60 steps
_README = dict(agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, init_pos=[60, 60], target_list=[[70, 200]])
_FAST = dict(agent_radius=15, agent_max_speed=60)
CASES = [
    dict(id='readme-folded', B=B, long=60, path='k_closed<1>', folded=True, gaze='Oxford', kw=dict(map_id=1, **_README)),
    dict(id='readme-safe_dist', B=B, long=60, path='k_closed<1>', folded=False, safe_dist=1.0, gaze='Oxford', kw=dict(map_id=1, **_README)),
    dict(id='agents-16', B=B, long=40, path='k_closed<1>', gaze='Oxford', kw=dict(agent_number=16, map_id=801, **CL._NEAR, **_FAST)),
    dict(id='agents-17', B=B, long=40, path='k_closed<2>', gaze='Oxford', kw=dict(agent_number=17, map_id=802, **CL._NEAR, **_FAST)),
    # blocks of 5 x 5 cells: dyn_full's plain loops, and the gate's marks over blocks wider than 3 x 3
    dict(id='radius-25', B=B, long=40, path='k_closed<1>', gaze='Oxford',
         kw=dict(agent_number=10, agent_radius=25, agent_max_speed=40, map_id=803, **CL._NEAR)),
    # 60 x 50 cells: the generic kernel, which defers nothing (max_flight_time 3 s = 30 steps: no episode outlasts the longer call)
    dict(id='map60x50', B=B, long=40, path='k_closed<0>', gaze='Oxford',
         kw=dict(agent_number=6, map_id=804, map_size=[600, 500], init_pos=[60, 60], target_list=[[200, 300]], max_flight_time=3, **_FAST)),
    # the non-split site (ph_gaze_stages<D2D_ST_ALL>): tests/test_gpu_hidden_obs.py, `lookahead-nomove`
    dict(id='lookahead-nomove', B=B, long=50, path='k_closed<1>', all_site=True, gaze='LookAhead',
         kw=dict(agent_number=16, map_id=730, init_pos=[250, 250], **_FAST)),
]


def _calls(pkg, oracle, case, mode, ref, hidden, every, edit=None):
    """the calls of one case; `edit(env)`: a change of the state made to all three envs before the first call"""
    from drone2d_amd import gaze as G
    policy = G.LookAhead(ref.params) if case['gaze'] == 'LookAhead' else None
    if edit:
        for env in (ref, hidden, every):
            edit(env)
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        t = 0
        for n in SHORT + (case['long'],):
            call = ref_call(pkg, ref, case, mode, policy, n)
            with every_step(True):
                every.closed_loop(n, **MODES[mode])
                every.sync()
            with every_step(False):
                hidden.closed_loop(n, **MODES[mode])
                hidden.sync()
            t += n
            tag = f"{case['id']} {mode} after step {t}"
            a, b = _snapshot(hidden), _snapshot(every)
            assert 's.gt' in a and 's.dyn_prev' in a
            _same({k: a[k] for k in ('s.gt', 's.dyn_prev')}, {k: b[k] for k in ('s.gt', 's.dyn_prev')}, tag)
            _same(a, b, tag)
            _assert_same(hidden, ref, tag)
            _assert_same(every, ref, tag + ' (every step)')
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    return call


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['id'])
def test_deferred_update_leaves_what_every_step_left(pkg, hip, oracle, spec, case, mode):
    p, ref = ref_env(pkg, oracle, case)
    hidden, every = _devices(pkg, hip, case, p, _worlds(ref))
    assert CL.closed_loop_path(hidden.cfg, hidden._plan) == case['path']
    if 'folded' in case:
        assert matches(spec, hidden.cfg, hidden._plan) == case['folded']
    if case.get('all_site'):
        assert hidden._plan.planner == pkg._abi.PLAN_NONE and hidden._plan.gaze != pkg._abi.GAZE_NONE
    call = _calls(pkg, oracle, case, mode, ref, hidden, every)
    # at least one env ended its episode on a step of the longer call that is not its last: under RESET it restarted inside the call
    n_mid = int(call['mid'].sum())
    print(f"{case['id']} {mode}: {n_mid} of {case['B']} envs ended an episode inside the {case['long']}-step call")
    assert n_mid >= 1, (case['id'], mode, n_mid)
    A = pkg._abi
    assert int((hidden.state.logical('gt') == A.DYNAMIC).sum()) > 0


def _crossed_cells(pkg, oracle, case, nsteps):
    """per env (i, j) or None: a free cell that an agent's block covers on steps 2 .. nsteps - 1 of the oracle's run, outside the blocks
    the run starts from and the blocks of its first and of its last step -- an agent crosses it only on steps a launch of `nsteps`
    steps would skip"""
    A = pkg._abi
    _, ref = ref_env(pkg, oracle, case)
    W, H = ref.cfg.W, ref.cfg.H

    def blocks(prev):
        out = set()
        for cx, cy, u in prev.reshape(-1, 3).tolist():
            out |= {(i, j) for i in range(max(cx - u, 0), min(cx + u + 1, W)) for j in range(max(cy - u, 0), min(cy + u + 1, H))}
        return out
    gt0, hist = ref.state.gt.clone(), [ref.state.dyn_prev.clone()]
    for _ in range(nsteps):
        ref.closed_loop(1)
        hist.append(ref.state.dyn_prev.clone())
    cells = []
    for e in range(ref.num_envs):
        mid = set().union(*[blocks(h[e]) for h in hist[2:-1]])
        cand = sorted(c for c in mid - blocks(hist[0][e]) - blocks(hist[1][e]) - blocks(hist[-1][e]) if gt0[e, c[0], c[1]] == A.UNOCCUPIED)
        cells.append(cand[0] if cand else None)
    return cells


GATE_CASE = dict(id='gate', B=B, long=40, path='k_closed<1>', gaze='Oxford',
                 kw=dict(agent_number=10, agent_radius=15, agent_max_speed=60, drone_max_speed=40, init_pos=[60, 60], target_list=[[70, 200]],
                         map_id=1))


@pytest.mark.parametrize('code', ['UNEXPLORED', 'DYNAMIC'])
@pytest.mark.parametrize('mode,where', [('continue', 'state'), ('reset', 'state'), ('reset', 'snapshot')])
def test_a_grid_that_fails_the_gate_equals_the_oracle(pkg, hip, oracle, code, mode, where):
    """One cell per env holds UNEXPLORED, or DYNAMIC outside every dyn_prev block, where an agent crosses it only on hidden steps of
    the first call: deferring would leave it as it is.  `state`: the live grid alone is edited -- under RESET the env fails the gate,
    is reset to a clean snapshot inside a later call and passes it.  `snapshot`: the snapshot is edited too -- every reset fails again.
    The first call has 40 steps here: the cell is crossed inside one launch."""
    A = pkg._abi
    case = dict(GATE_CASE)
    cells = _crossed_cells(pkg, oracle, case, case['long'])
    assert sum(c is not None for c in cells) >= B // 2
    value = getattr(A, code)

    def edit(env):
        for st in (env.state, env.init_state) if where == 'snapshot' else (env.state,):
            for e, c in enumerate(cells):
                if c is not None:
                    st.gt[e, c[0], c[1]] = value
    p, ref = ref_env(pkg, oracle, case)
    hidden, every = _devices(pkg, hip, case, p, _worlds(ref))
    assert CL.closed_loop_path(hidden.cfg, hidden._plan) == case['path']
    for env in (ref, hidden, every):
        edit(env)
    oracle.lib.d2d_oracle_set_threads(8)
    try:
        t = 0
        for n in (case['long'], 1, case['long']):
            ref.closed_loop(n, **MODES[mode])
            with every_step(True):
                every.closed_loop(n, **MODES[mode])
            with every_step(False):
                hidden.closed_loop(n, **MODES[mode])
            t += n
            tag = f'{code} {mode} {where} after step {t}'
            _same(_snapshot(hidden), _snapshot(every), tag)
            _assert_same(hidden, ref, tag)
            if t == case['long'] and mode == 'continue':
                # the edit did what it is there for: the every-step rule cleared the cells an agent crossed
                g = ref.state.gt
                assert all(int(g[e, c[0], c[1]]) == A.UNOCCUPIED for e, c in enumerate(cells) if c is not None)
    finally:
        oracle.lib.d2d_oracle_set_threads(1)
    if mode == 'reset':
        assert int((ref.state.counters[:, A.C_STEPS] < t).sum()) >= B // 2      # envs restarted inside the calls
