"""Episode tables on the device: the world build with D2D_WE_REDRAW against host_init.init_world(redraw=True) byte for byte, plain and
masked; d2d_stream_assign_table against its Python model (tests/table_model.py) over the slot counts, flag patterns and cursor
positions at which the scan takes another path; whole table streams against ONE batch of the same worlds, host-built, in all four
cells with and without the redraw; a refilled slot against a fresh env of its episode in every tensor; and the reference's recorded
validation episodes (tests/golden/validation_episodes.npz) through runner.EpisodeStream(episodes=...).  Every comparison is exact."""
import functools
from itertools import product

import numpy as np
import pytest
import torch

import stream_model as SM
import table_model as TM
import world_cases as WC
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu

STARTS = [(40, 40), (460, 250), (250, 460), (40, 250), (460, 460)]
TARGETS = [[(250, 250), (460, 40)], [(40, 40), (250, 460)], [(460, 460), (40, 250)]]
WORLDS = {                                   # 16 worlds each, one launch: per-env map id, start position and two targets
    'n0': dict(agent_number=0),
    'n3': dict(agent_number=3),
    'n70-two-lane-passes': dict(agent_number=70, agent_radius=5),
    'n172-random_map_0': dict(agent_number=50, static_map='maps/random_map_0.npy'),     # 688 words: always past a regeneration
    'random-radius': dict(agent_radius=-1, agent_max_speed=20),
    'obstacle_map-pillars': dict(static_map='maps/obstacle_map.npy', pillar_number=3, agent_radius=15),
}


def world_params(pkg, name):
    return [pkg.Params(planner='NoMove', var_cam=2, map_id=7 * e + 1, init_pos=STARTS[e % 5], target_list=TARGETS[e % 3], **WORLDS[name])
            for e in range(16)]


@functools.lru_cache(maxsize=None)
def host_worlds(name):
    import drone2d_amd as pkg
    from drone2d_amd import host_init
    return tuple(host_init.init_world(pkg.with_defaults(p), redraw=True) for p in world_params(pkg, name))


def _device_fields(dw):
    out = {f: dw.state.t[f].cpu().numpy() for f in WC.FIELDS}
    out['rng'] = dw.state.t['rng'].cpu().numpy()
    out.update(tracker_radius=dw.tracker_radius.numpy(), obstacles=dw.obstacles, status=dw.status)
    return out


def _poison(t):
    t.view(torch.uint8).fill_(0xA5)


@pytest.mark.parametrize('layout', ['rowmajor', 'tiled'])
@pytest.mark.parametrize('name', list(WORLDS))
def test_redrawn_worlds_are_init_world(pkg, hip, name, layout):
    from drone2d_amd import host_init, vec_env
    from drone2d_amd.state import BatchState, WORLD_FIELDS
    plist = world_params(pkg, name)
    tile = 16 if layout == 'tiled' else 0
    exp = WC.stack_worlds(pkg, list(host_worlds(name)), tile)
    dw = vec_env.build_worlds_device_of(plist, backend=hip, grid_layout=layout, redraw=True)
    WC.assert_equal(_device_fields(dw), exp, with_rng=True)
    N = exp['agents'].shape[2]
    assert N == {'n0': 0, 'n3': 3, 'n70-two-lane-passes': 70, 'n172-random_map_0': 172, 'random-radius': 10, 'obstacle_map-pillars': 24}[name]
    if N:                                    # the redraw moved something: the plain build differs in the velocities alone
        plain = vec_env.build_worlds_device_of(plist, backend=hip, grid_layout=layout)
        a, b = dw.state.t['agents'].cpu().numpy(), plain.state.t['agents'].cpu().numpy()
        assert not np.array_equal(a[:, A.A_VX:A.A_VY + 1], b[:, A.A_VX:A.A_VY + 1])
        keep = [A.A_PX, A.A_PY, A.A_R, A.A_R2]
        assert np.array_equal(a[:, keep], b[:, keep])
        for f in ('gt', 'rng', 'dyn_prev', 'drone', 'targets'):
            assert torch.equal(dw.state.t[f], plain.state.t[f]), f
    # the masked build of the same worlds, alternating bytes: the slots of the mask are the worlds above, the others untouched
    inp = vec_env.world_inputs(plist, redraw=True)
    B, P = 16, inp['P']
    cfg = host_init.derive_cfg(pkg.with_defaults(plist[0]), B=B, N=N, T=inp['T'], grid_tile=tile)
    st = BatchState(cfg, hip.device)
    dev = st.device
    up = {n: torch.from_numpy(inp[n].view(np.int32) if n == 'map_id' else inp[n]).to(dev) for n in ('unit', 'cells', 'map_id', 'env_par', 'env_tgt')}
    up['tracker_radius'] = torch.zeros((B, N), dtype=torch.float64, device=dev)
    up['obstacles'] = torch.zeros((B, P, 3), dtype=torch.int32, device=dev)
    up['status'] = torch.zeros(B, dtype=torch.int32, device=dev)
    outs = ('tracker_radius', 'obstacles', 'status')
    written = [n for n in WORLD_FIELDS if n in st.t] + ['flags']
    assert 'rng' in written and 'agents' in written
    for n in written:
        _poison(st.t[n])
    for n in outs:
        _poison(up[n])
    before = {n: st.t[n].clone() for n in written}
    before.update({n: up[n].clone() for n in outs})
    mask = torch.tensor([1, 0] * 8, dtype=torch.uint8, device=dev)
    spec = vec_env.world_spec(inp, tile, lambda n: up[n].data_ptr() if up[n].numel() else st._dummy.data_ptr())
    hip.build_worlds_masked(spec, st.struct(), mask)
    hip.sync()
    for n in written + list(outs):
        got = up[n] if n in outs else st.t[n]
        want = {'tracker_radius': dw.tracker_radius.to(dev), 'obstacles': torch.from_numpy(dw.obstacles).to(dev).int(),
                'status': torch.from_numpy(dw.status).to(dev), 'flags': torch.zeros_like(st.flags)}.get(n)
        if want is None:
            want = dw.state.t[n]
        for e in range(B):
            ref = want[e] if e % 2 == 0 else before[n][e]
            assert torch.equal(got[e].reshape(-1).view(torch.uint8), ref.reshape(-1).view(torch.uint8)), (n, e)


def test_a_launch_mixes_redrawn_and_plain_envs(pkg, hip):
    """D2D_WE_REDRAW is per env: odd envs of one launch without it are the plain worlds"""
    from drone2d_amd import vec_env
    name = 'n70-two-lane-passes'
    plist = world_params(pkg, name)
    both = {r: vec_env.build_worlds_device_of(plist, backend=hip, redraw=r) for r in (False, True)}
    inp = vec_env.world_inputs(plist, redraw=True)
    inp['env_par'][1::2, A.WE_REDRAW] = 0.0
    import unittest.mock as mock
    with mock.patch.object(vec_env, 'world_inputs', lambda *a, **k: inp):
        mixed = vec_env.build_worlds_device_of(plist, backend=hip)
    for f in mixed.state.t:
        for e in range(16):
            assert torch.equal(mixed.state.t[f][e], both[e % 2 == 0].state.t[f][e]), (f, e)


# ---------------------------------------------------------------------------------------------------------------- assignment
@pytest.mark.parametrize('B', [5, 1030], ids=['B5', 'B1030-two-strides'])
def test_assign_table_against_the_model(hip, B):
    rs = np.random.RandomState(B)
    dev, T = hip.device, 2
    done_of = {'none': np.zeros(B, bool), 'all': np.ones(B, bool), 'alternating': np.arange(B) % 2 == 0}
    for (pattern, done), (M, cursor) in product(done_of.items(), ((B - 2, B - 2), (B, B), (3 * B, B), (3 * B, 3 * B - 2), (3 * B, 3 * B),
                                                                  (B + B // 2, B + 1), (0, 0))):
        flags = rs.randint(0, 3, size=(B, 4)).astype(np.uint8)
        flags[:, A.F_DONE] = done
        slot = rs.permutation(max(B, M))[:B].astype(np.int32)
        slot[rs.rand(B) < 0.1] = -1                                    # retired by an earlier call
        ep_map_id = rs.randint(0, 2 ** 32, size=M, dtype=np.uint64).astype(np.uint32)
        ep_par, ep_tgt = rs.rand(M, A.WORLDS_ENV_F), rs.rand(M, T, 2)
        map_id, par, tgt = rs.randint(0, 2 ** 32, size=B, dtype=np.uint64).astype(np.uint32), rs.rand(B, A.WORLDS_ENV_F), rs.rand(B, T, 2)
        refill, counts = np.full(B, 9, np.uint8), np.array([cursor, 5], np.int64)
        d = {k: torch.from_numpy(v.view(np.int32).copy() if v.dtype == np.uint32 else v.copy()).to(dev)
             for k, v in dict(flags=flags, slot=slot, ep_map_id=ep_map_id, ep_par=ep_par, ep_tgt=ep_tgt, map_id=map_id, par=par, tgt=tgt,
                              refill=refill, counts=counts).items()}
        hip.stream_assign_table(d['flags'], d['ep_map_id'], d['ep_par'], d['ep_tgt'], d['slot'], d['map_id'], d['par'], d['tgt'],
                                d['refill'], d['counts'])
        hip.sync()
        TM.assign_table(flags, slot, map_id, par, tgt, refill, counts, ep_map_id, ep_par, ep_tgt)
        case = (pattern, M, cursor)
        for k, want in dict(slot=slot, map_id=map_id.view(np.int32), par=par, tgt=tgt, refill=refill, counts=counts, flags=flags,
                            ep_par=ep_par, ep_tgt=ep_tgt).items():
            got = d[k].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (case, k)       # every byte, of the slots that got nothing too
        if pattern == 'all' and cursor < M:
            assert refill.any()


# ---------------------------------------------------------------------------------------------------------------- streams
COMMON = dict(agent_number=3, agent_radius=15, agent_max_speed=40, drone_max_speed=40, max_flight_time=4)
CELLS = {
    'Primitive-Oxford-CVM': dict(planner='Primitive', gaze_method='Oxford'),
    'Primitive-LookAhead-RVO': dict(planner='Primitive', gaze_method='LookAhead', motion_profile='RVO', pillar_number=2),
    'Jerk-Owl-CVM': dict(planner='Jerk_Primitive', gaze_method='Owl'),
    'Jerk-LookAhead-RVO': dict(planner='Jerk_Primitive', gaze_method='LookAhead', motion_profile='RVO'),
}
PAIRS = [((40, 40), (110, 60)), ((460, 250), (400, 320)), ((250, 460), (250, 40)), ((40, 250), (460, 460)), ((250, 250), (300, 200)),
         ((460, 460), (250, 250)), ((40, 460), (100, 400)), ((250, 40), (40, 40))]
M, SLOTS = 23, 4


def table_of(pkg, cell, m=M):
    rows = [(mid, s, t) for mid, (s, t) in product((5, 0, 2), PAIRS)][:m]
    return [pkg.Params(**dict(dict(COMMON, **CELLS[cell]), map_id=mid, init_pos=s, target_list=[t])) for mid, s, t in rows]


_batch_rows = {}


def batch_rows(pkg, hip, cell, redraw):
    """the rows of ONE batch of the table's worlds, host-built, run by the cell's batch loop: computed once"""
    if (cell, redraw) not in _batch_rows:
        table = table_of(pkg, cell)
        rows = TM.rows_of_worlds(table[0], table, redraw, backend=hip)
        assert len({r[12] for r in rows}) > 2, [r[12] for r in rows]        # the episodes end at different steps
        _batch_rows[(cell, redraw)] = rows
    return _batch_rows[(cell, redraw)]


@pytest.mark.parametrize('redraw', [False, True], ids=['plain', 'redraw'])
@pytest.mark.parametrize('cell', list(CELLS))
def test_table_stream_rows_are_one_batchs_rows(pkg, hip, cell, redraw):
    from drone2d_amd import runner
    import stream_backend as SB
    table = table_of(pkg, cell)
    want = batch_rows(pkg, hip, cell, redraw)
    for every in (1, 5, 64):
        xs = runner.EpisodeStream(table[0], episodes=table, slots=SLOTS, backend=hip, redraw_agents=redraw)
        rows = xs.run(refill_every=every)
        assert SB.same_rows(rows, want), (every, [k for k in range(M) if not SB.same_rows([rows[k]], [want[k]])])
        assert xs.build_failed == [] and xs.steps_run % every == 0
    assert [r[3] for r in rows] == [5] * 8 + [0] * 8 + [2] * 7 and [r[10] for r in rows[:8]] == [s for s, _ in PAIRS]
    if redraw:
        assert not SB.same_rows(want, batch_rows(pkg, hip, cell, False))


@pytest.mark.parametrize('redraw', [False, True], ids=['plain', 'redraw'])
@pytest.mark.parametrize('cell', list(CELLS))
def test_a_refilled_slot_is_a_fresh_env_of_its_episode(pkg, hip, cell, redraw):
    """4 slots, the first refill, taken after every slot's episode has ended (48 > 41 steps): slot e then holds episode 4 + e, and is
    env 0 of a new one-env VecDrone2DEnv of that row in every tensor"""
    from drone2d_amd import runner, vec_env
    from test_gpu_episode_stream import _tensors
    table = table_of(pkg, cell, 8)
    xs = runner.EpisodeStream(table[0], episodes=table, slots=SLOTS, backend=hip, redraw_agents=redraw)
    env = xs.env
    finished, refill = next(env.stream_rounds(refill_every=48, episodes=table))
    env.sync()
    assert finished == 4 and refill.tolist() == [1, 1, 1, 1]
    for e in (0, 3):
        q = table[4 + e]
        fresh = vec_env.VecDrone2DEnv(q, 1, backend=hip, planner=q.planner, worlds='device', device_plugins=True, gaze=q.gaze_method,
                                      redraw_agents=redraw)
        got, exp = _tensors(env, e), _tensors(fresh, 0)
        assert set(got) == set(exp)
        for k in sorted(got):
            assert torch.equal(got[k].reshape(-1).view(torch.uint8).cpu(), exp[k].reshape(-1).view(torch.uint8).cpu()), (e, k)
        assert float(got['s.drone'][A.D_X]) == q.init_position[0] and got['s.targets'][0].tolist() == list(q.target_list[0])


@pytest.mark.parametrize('m', [0, 1, 3])
def test_fewer_episodes_than_slots(pkg, hip, m):
    from drone2d_amd import runner
    import stream_backend as SB
    cell = 'Primitive-Oxford-CVM'
    table = table_of(pkg, cell, m)
    xs = runner.EpisodeStream(table_of(pkg, cell, 1)[0], episodes=table, slots=SLOTS, backend=hip, redraw_agents=True)
    rows = xs.run(refill_every=16)
    assert SB.same_rows(rows, batch_rows(pkg, hip, cell, True)[:m])
    assert xs.records.shape == (m, A.STREAM_ROW_F)
    assert xs.env.state.counters[m:, A.C_STEPS].tolist() == [0] * (SLOTS - m)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_the_references_validation_episodes(pkg, hip):
    """the recorded episodes of script/validation_speed.py and validation_size.py, cell by cell through EpisodeStream(episodes=...)
    over one slot (so every episode but a cell's first is a refill): the rows are the reference's"""
    from drone2d_amd import runner
    eps, tie = TM.golden()
    seen = 0
    for idx, plist, redraw, speed in TM.golden_cells(pkg):
        xs = runner.EpisodeStream(plist[0], episodes=plist, slots=1, backend=hip, redraw_agents=redraw, agent_speed=speed, jerk_tie=tie)
        rows = xs.run(refill_every=32)
        for i, r in zip(idx, rows):
            c = eps[i]['cfg']
            assert TM.same_numbers(r, eps[i]['row']), (i, TM.row_numbers(r).tolist(), eps[i]['row'].tolist())
            assert r[:12] == (plist[0].gaze_method, plist[0].planner, 'CVM', c['map_id'], c['agent_radius'], c['agent_number'], 0,
                              -1 if redraw else c['agent_max_speed'], c['drone_max_speed'], 0, tuple(c['start']), tuple(c['target']))
            seen += 1
    assert seen == len(eps) == 11
