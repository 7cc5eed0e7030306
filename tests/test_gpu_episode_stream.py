"""The launches of include/d2d_worlds_stream.h on the device: harvest and assign against the numpy model (tests/stream_model.py) over
the slot counts and grid layouts at which the kernels take another path, the masked build against d2d_worlds_build, a refilled slot
against a freshly constructed env in every tensor, and whole streams against the batch runners' rows.  Every comparison is exact."""
import copy

import numpy as np
import pytest
import torch

import stream_model as SM
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu

GRIDS = {'50x50-rowmajor': (50, 50, 'rowmajor'), '29x31-rowmajor': (29, 31, 'rowmajor'), '30x29-tiled': (30, 29, 'tiled')}
SLOT_COUNTS = (1, 63, 64, 65, 1100)           # 1100 crosses the assign workgroup's stride of 1024: the scan's carry


def _state(pkg, hip, B, W, H, layout, **kw):
    from drone2d_amd import host_init, vec_env
    from drone2d_amd.params import with_defaults
    from drone2d_amd.state import BatchState
    p = with_defaults(pkg.Params(planner='NoMove', map_size=[10 * W, 10 * H], map_scale=10, agent_number=2, **kw))
    cfg = host_init.derive_cfg(p, B=B, N=2, T=1, grid_tile=vec_env._grid_tile(p, hip, layout))
    return BatchState(cfg, hip.device)


def _patterns(rs, B):
    """name -> (done [B] bool, slot_episode [B], cursor, M)"""
    third = rs.rand(B) < 1 / 3
    if B <= 2:
        third[:] = True
    perm = rs.permutation(B).astype(np.int32)              # the slots play episodes 0 .. B - 1 in some order; the cursor stands at B
    big = 3 * B + 10
    retired = perm.copy()
    retired[third & (rs.rand(B) < 0.5)] = -1                # some of the done ones were retired by an earlier call
    retired[(~third) & (rs.rand(B) < 0.1)] = -1             # (a retired slot is always done; one that is not stays unharvested too)
    n = int(third.sum())
    return {
        'none': (np.zeros(B, bool), perm, B, big),
        'all': (np.ones(B, bool), perm, B, big),
        'third': (third, perm, B, big),
        'runs-dry': (third, perm, B, B + n // 2),          # fewer episodes left than slots done: the rest retire
        'exactly-dry': (np.ones(B, bool), perm, B, B),      # the cursor stands at M already: every done slot retires
        'retired-among-done': (third, retired, B, big),
    }


@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('B', SLOT_COUNTS, ids=[f'B{b}' for b in SLOT_COUNTS])
def test_harvest_and_assign_against_the_model(pkg, hip, B, grid):
    W, H, layout = GRIDS[grid]
    st = _state(pkg, hip, B, W, H, layout)
    assert (st.cfg.grid_tile == 16) == (layout == 'tiled')
    rs = np.random.RandomState(B * 31 + W)
    dev = st.device
    # random bytes everywhere, the tile padding included; values >= 128 among them
    dmap = rs.randint(0, 256, size=tuple(st.dmap.shape)).astype(np.uint8)
    dmap[rs.rand(*dmap.shape) < 0.4] = 0
    st.dmap.copy_(torch.from_numpy(dmap))
    assert (dmap >= 128).any() and (W * H) % 4 == {'50x50-rowmajor': 0, '29x31-rowmajor': 3, '30x29-tiled': 2}[grid]
    counters = rs.randint(0, 1000, size=(B, A.CF)).astype(np.int32)
    st.counters.copy_(torch.from_numpy(counters))
    logical = st.logical('dmap').cpu().numpy()
    struct = st.struct()
    for name, (done, slot_episode, cursor, M) in _patterns(rs, B).items():
        flags = rs.randint(0, 3, size=(B, 4)).astype(np.uint8)
        flags[:, A.F_DONE] = done
        st.flags.copy_(torch.from_numpy(flags))
        d_slot = torch.from_numpy(slot_episode.copy()).to(dev)
        d_rows = torch.full((M, A.STREAM_ROW_F), SM.SENTINEL, dtype=torch.int32, device=dev)
        d_map = torch.full((B,), 77, dtype=torch.int32, device=dev)
        d_refill = torch.full((B,), 9, dtype=torch.uint8, device=dev)
        d_counts = torch.tensor([cursor, 5], dtype=torch.int64, device=dev)
        map_id0 = 2 ** 32 - M if name == 'all' else 1000        # 'all': map ids up to 2**32 - 1
        hip.stream_harvest(st.cfg, struct, d_slot, d_rows)
        hip.stream_assign(st.flags, M, map_id0, d_slot, d_map, d_refill, d_counts)
        hip.sync()
        # the model on copies
        rows = np.full((M, A.STREAM_ROW_F), SM.SENTINEL, dtype=np.int64)
        slot, map_id, refill, counts = slot_episode.copy(), np.full(B, 77, np.uint32), np.full(B, 9, np.uint8), np.array([cursor, 5], np.int64)
        SM.harvest(SM.records(counters, flags, logical), flags, slot, rows)
        SM.assign(flags, slot, map_id, refill, counts, M, map_id0)
        assert np.array_equal(d_rows.cpu().numpy(), rows), name
        assert np.array_equal(d_slot.cpu().numpy(), slot), name
        assert np.array_equal(d_map.cpu().numpy().view(np.uint32), map_id), name
        assert np.array_equal(d_refill.cpu().numpy(), refill), name
        assert d_counts.tolist() == counts.tolist(), name
        assert torch.equal(st.flags.cpu(), torch.from_numpy(flags)), name         # the done bytes stay, a retired slot's included
        # what the pattern is for
        h = SM.harvested(flags, slot_episode)
        assert int((rows[:, 0] != SM.SENTINEL).sum()) == int(h.sum()) == counts[1] - 5, name
        if name in ('runs-dry', 'exactly-dry') and h.any():
            assert counts[0] == M and (slot[h] == -1).any() and int(refill.sum()) == M - cursor, name


def _poison(t):
    t.view(torch.uint8).fill_(0xA5)


def test_masked_build_writes_the_refilled_slots_and_nothing_else(pkg, hip):
    """9 slots, 10 agents + the static map's, 3 pillars, var_cam != 0 (the stream's key is a world field too)"""
    from drone2d_amd import host_init, vec_env
    from drone2d_amd.params import with_defaults
    from drone2d_amd.state import BatchState, WORLD_FIELDS
    B = 9
    p = with_defaults(pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20, pillar_number=3,
                                 static_map='maps/obstacle_map.npy', var_cam=2))
    ids = [100 + 7 * e for e in range(B)]
    pattern = np.array([1, 1, 0, 0, 1, 0, 0, 1, 1], dtype=np.uint8)      # the first, the last, neighbours, lone ones
    want = vec_env.build_worlds_device_of([p], backend=hip, map_ids=ids)
    inp = vec_env.world_inputs([p], map_ids=ids)
    N, P = inp['N'], inp['P']
    cfg = host_init.derive_cfg(p, B=B, N=N, T=inp['T'], grid_tile=0)
    st = BatchState(cfg, hip.device)
    dev = st.device
    up = {n: torch.from_numpy(inp[n].view(np.int32) if n == 'map_id' else inp[n]).to(dev) for n in ('unit', 'cells', 'map_id', 'env_par', 'env_tgt')}
    up['tracker_radius'] = torch.zeros((B, N), dtype=torch.float64, device=dev)
    up['obstacles'] = torch.zeros((B, P, 3), dtype=torch.int32, device=dev)
    up['status'] = torch.zeros(B, dtype=torch.int32, device=dev)
    out_names = ('tracker_radius', 'obstacles', 'status')
    written = [n for n in WORLD_FIELDS if n in st.t] + ['flags']
    assert 'rng' in written
    for n in written:
        _poison(st.t[n])
    for n in out_names:
        _poison(up[n])
    before = {n: st.t[n].clone() for n in written}
    before.update({n: up[n].clone() for n in out_names})
    spec = vec_env.world_spec(inp, 0, lambda n: up[n].data_ptr())
    hip.build_worlds_masked(spec, st.struct(), torch.from_numpy(pattern).to(dev))
    hip.sync()

    def check(refilled, capped=()):
        for n in written + list(out_names):
            got = up[n] if n in out_names else st.t[n]
            exp = {'tracker_radius': want.tracker_radius.to(dev), 'obstacles': torch.from_numpy(want.obstacles).to(dev).int(),
                   'status': torch.from_numpy(want.status).to(dev), 'flags': torch.zeros_like(st.flags)}.get(n)
            if exp is None:
                exp = want.state.t[n]
            for e in range(B):
                if e in capped:
                    ref = torch.zeros_like(got[e])
                    if n == 'status':
                        ref = ref + A.WORLD_CAP
                    if n == 'flags':
                        ref[A.F_DONE] = 1
                elif e in refilled:
                    ref = exp[e]
                else:
                    ref = before[n][e]
                assert torch.equal(got[e].reshape(-1).view(torch.uint8), ref.reshape(-1).view(torch.uint8)), (n, e)

    refilled = set(np.nonzero(pattern)[0].tolist())
    check(refilled)
    assert (want.status == A.WORLD_OK).all()
    # one slot again, with a max_attempts too small to place its agents: status CAP, done byte set, fields zero; nothing else moves
    small = dict(inp, max_attempts=5)
    spec = vec_env.world_spec(small, 0, lambda n: up[n].data_ptr())
    one = torch.zeros(B, dtype=torch.uint8, device=dev)
    one[4] = 1
    hip.build_worlds_masked(spec, st.struct(), one)
    hip.sync()
    check(refilled - {4}, capped={4})


@pytest.mark.parametrize('B,row', [(1, (3,)), (9, (5, 7)), (300, (1585, 12))], ids=['B1-3words', 'B9-35doubles', 'B300-1585x12doubles'])
def test_clear_zeroes_the_refilled_rows_and_nothing_else(hip, B, row):
    rs = np.random.RandomState(B)
    dt = torch.int32 if len(row) == 1 else torch.float64
    t = torch.empty((B,) + row, dtype=dt, device=hip.device)
    _poison(t)
    before = t.clone()
    mask = (rs.rand(B) < 0.4).astype(np.uint8)
    mask[0] = mask[-1] = 1
    refill = torch.from_numpy(mask).to(hip.device)
    hip.stream_clear(t, refill)
    hip.sync()
    want = torch.where(refill.bool().view((-1,) + (1,) * len(row)), torch.zeros_like(before), before)
    assert torch.equal(t.view(torch.uint8), want.view(torch.uint8))
    hip.stream_clear(t, torch.zeros_like(refill))
    hip.sync()
    assert torch.equal(t.view(torch.uint8), want.view(torch.uint8))


COMMON = dict(agent_number=25, agent_radius=15, agent_max_speed=40, drone_max_speed=40, max_flight_time=4, map_id=3,
              target_list=[[90, 90]])
CELLS = {
    'Primitive-Oxford-CVM': dict(planner='Primitive', gaze_method='Oxford'),
    'Primitive-LookAhead-RVO-3pillars': dict(planner='Primitive', gaze_method='LookAhead', motion_profile='RVO', pillar_number=3),
    'Jerk-Owl-CVM': dict(planner='Jerk_Primitive', gaze_method='Owl'),
    'Jerk-LookAhead-RVO': dict(planner='Jerk_Primitive', gaze_method='LookAhead', motion_profile='RVO'),
}
FRESH = {
    'Primitive-Owl-CVM-varcam2': dict(planner='Primitive', gaze_method='Owl', var_cam=2),
    'Primitive-LookAhead-RVO-3pillars': CELLS['Primitive-LookAhead-RVO-3pillars'],
    'Jerk-Owl-CVM-varcam2': dict(planner='Jerk_Primitive', gaze_method='Owl', var_cam=2),
    'Jerk-LookAhead-RVO': CELLS['Jerk-LookAhead-RVO'],
}
NOT_PER_SLOT = ('launch_args',)      # one block of launch arguments per batch: there is no row of a slot to compare


def _tensors(env, e):
    out = {'s.' + k: v[e] for k, v in env.state.t.items()}
    if env.plugins is not None:
        out.update({'p.' + k: v[e] for k, v in env.plugins.t.items() if k not in NOT_PER_SLOT})
        out['p.trk_radius0'] = env.plugins.trk_radius0[e]
    if env.jerk is not None:
        out.update({'j.' + k: v[e] for k, v in env.jerk.t.items()})
        out['j.trk_radius0'] = env.jerk.trk_radius0[e]
    if env.gaze_state is not None and env.gaze_state.owl_state is not None:
        out['g.owl_state'] = env.gaze_state.owl_state[e]
    return out


@pytest.mark.parametrize('cell', list(FRESH))
def test_a_refilled_slot_is_a_fresh_env(pkg, hip, cell):
    """4 slots, the first refill of a stream, taken after every slot's episode has ended (48 > 41 steps): slot e then holds episode
    4 + e, and is env 0 of a new one-env VecDrone2DEnv of that map id in every tensor"""
    from drone2d_amd import runner, vec_env
    p = pkg.Params(**dict(COMMON, **FRESH[cell]))
    xs = runner.EpisodeStream(p, 8, 4, backend=hip)
    env = xs.env
    finished, refill = next(env.stream_rounds(8, refill_every=48))
    env.sync()
    assert finished == 4 and refill.tolist() == [1, 1, 1, 1]
    names = set(_tensors(env, 0))
    assert {'s.rng', 's.rng_draws'} <= names if 'varcam2' in cell else 's.rng' not in names
    assert ('p.owl_state' in names or 'g.owl_state' in names) == ('Owl' in cell)
    assert {'s.agent_vel', 's.agent_vel_out', 's.pillars'} <= names if 'RVO' in cell else 's.agent_vel' not in names
    assert {'p.traj', 'p.traj_box', 'p.nodes', 'p.hash'} <= names if 'Primitive-' in cell else 'p.traj' not in names
    if env.plugins is not None:          # the episodes that ended left something there for the refill to clear
        assert bool(env.plugins.t['plan_stat'].any()) is False and int(xs.env.stream_rows[:4, 0].min()) > 0
    for e in (0, 3):
        q = copy.copy(xs.params)
        q.map_id = p.map_id + 4 + e
        fresh = vec_env.VecDrone2DEnv(q, 1, backend=hip, planner=q.planner, worlds='device', device_plugins=True, gaze=q.gaze_method)
        got, exp = _tensors(env, e), _tensors(fresh, 0)
        assert set(got) == set(exp)
        for k in sorted(got):
            assert torch.equal(got[k].reshape(-1).view(torch.uint8).cpu(), exp[k].reshape(-1).view(torch.uint8).cpu()), (e, k)


_batch_rows = {}


def _rows_of_the_batch_runner(pkg, hip, cell):
    from drone2d_amd import runner
    if cell not in _batch_rows:
        p = pkg.Params(**dict(COMMON, **CELLS[cell]))
        cls = runner.ExperimentBatch if cell == 'Primitive-Oxford-CVM' else runner.SteppedExperimentBatch
        rows = cls(p, 24, backend=hip, device_worlds=True).run()
        assert len({r[12] for r in rows}) > 2                  # the episodes end at different steps
        _batch_rows[cell] = rows
    return _batch_rows[cell]


def _same_rows(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((u != u and v != v) or u == v for u, v in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize('cell,refill_every', [(c, 16) for c in CELLS] + [('Jerk-Owl-CVM', 1)],
                         ids=[f'{c}-24over8-every16' for c in CELLS] + ['Jerk-Owl-CVM-24over8-every1'])
def test_streamed_rows_are_the_batch_rows(pkg, hip, cell, refill_every):
    from drone2d_amd import runner
    p = pkg.Params(**dict(COMMON, **CELLS[cell]))
    xs = runner.EpisodeStream(p, 24, 8, backend=hip)
    rows = xs.run(refill_every=refill_every)
    want = _rows_of_the_batch_runner(pkg, hip, cell)
    assert _same_rows(rows, want), [k for k in range(24) if not _same_rows([rows[k]], [want[k]])]
    assert xs.build_failed == [] and xs.steps_run % refill_every == 0
