"""Episode tables without a GPU (VecDrone2DEnv.stream_episodes(episodes=...), runner.EpisodeStream(episodes=...),
runner.ValidationStudy): the refusals name their field and row, the study's grid is the scripts', the model of
d2d_stream_assign_table agrees with the model of d2d_stream_assign on a table of consecutive map ids, a table stream's rows are the
rows of one batch of the same worlds in all four cells, and include/d2d_worlds_table.h agrees with its ctypes binder."""
import copy
import ctypes as C
import os
import re
from itertools import product

import numpy as np
import pytest
import torch

import stream_model as SM
import table_model as TM
from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'd2d_worlds_table.h')).read()

COMMON = dict(agent_number=3, agent_radius=15, agent_max_speed=40, drone_max_speed=40, max_flight_time=4)
CELLS = {
    'Primitive-CVM': dict(planner='Primitive', gaze_method='Oxford'),
    'Primitive-RVO': dict(planner='Primitive', gaze_method='Oxford', motion_profile='RVO'),
    'Jerk-CVM': dict(planner='Jerk_Primitive', gaze_method='Owl'),
    'Jerk-RVO': dict(planner='Jerk_Primitive', gaze_method='LookAhead', motion_profile='RVO'),
}
PAIRS = [((40, 40), (110, 60)), ((460, 250), (400, 320)), ((250, 460), (250, 40)), ((40, 250), (460, 460))]     # two goals within reach


def table_of(pkg, cell, M, **kw):
    """M episodes drawn from 3 maps x the (start, target) pairs, as Params"""
    rows = [(m, s, t) for m, (s, t) in product((5, 0, 2), PAIRS)][:M]
    return [pkg.Params(**dict(dict(COMMON, **CELLS[cell]), map_id=m, init_pos=s, target_list=[t], **kw)) for m, s, t in rows]


# ---------------------------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize('redraw', [False, True], ids=['plain', 'redraw'])
@pytest.mark.parametrize('cell', list(CELLS))
def test_table_stream_rows_are_the_batch_rows(pkg, cell, redraw):
    table = table_of(pkg, cell, 9)
    want = TM.rows_of_worlds(table[0], table, redraw)
    assert len({r[12] for r in want}) > 1 and [r[3] for r in want] == [5] * 4 + [0] * 4 + [2]
    assert [r[10] for r in want[:4]] == [p[0] for p in PAIRS]
    for every in (1, 5, 64):
        xs = TM.table_stream_of(table[0], table, 4, redraw_agents=redraw)
        assert SM_same(xs.run(refill_every=every), want), every
        assert xs.build_failed == []


def SM_same(a, b):
    import stream_backend as SB
    return SB.same_rows(a, b)


@pytest.mark.parametrize('m', [0, 1, 3])
def test_fewer_episodes_than_slots(pkg, m):
    table = table_of(pkg, 'Jerk-CVM', m)
    base = table_of(pkg, 'Jerk-CVM', 1)[0]
    xs = TM.table_stream_of(base, table, 4, redraw_agents=True)
    rows = xs.run()
    assert SM_same(rows, TM.rows_of_worlds(base, table, True) if m else [])
    assert xs.records.shape == (m, A.STREAM_ROW_F)
    assert xs.env.state.counters[m:, A.C_STEPS].tolist() == [0] * (4 - m)


def test_triples_over_the_envs_own_params(pkg):
    table = table_of(pkg, 'Primitive-CVM', 5)
    triples = [(p.map_id, p.init_position, p.target_list) for p in table]
    a = TM.table_stream_of(table[0], table, 2).run()
    b = TM.table_stream_of(table[0], triples, 2).run()
    assert SM_same(a, b) and [r[11] for r in b] == [p.target_list[0] for p in table]


def test_agent_speed_column(pkg):
    table = table_of(pkg, 'Primitive-CVM', 3)
    rows = TM.table_stream_of(table[0], table, 2, redraw_agents=True, agent_speed=-1).run()
    assert [r[7] for r in rows] == [-1] * 3 and all(len(r) == 22 for r in rows)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _env(pkg, cell='Primitive-CVM', slots=2, M=4, **kw):
    table = table_of(pkg, cell, M, **kw)
    return TM.table_stream_of(table[0], table, slots).env, table


def _changed(p, **kw):
    q = copy.copy(pkg_with_defaults(p))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def pkg_with_defaults(p):
    from drone2d_amd.params import with_defaults
    return with_defaults(p)


@pytest.mark.parametrize('field,value', [
    ('map_size', [600, 500]), ('map_scale', 5), ('agent_number', 4), ('pillar_number', 2), ('static_map', 'maps/obstacle_map.npy'),
    ('drone_radius', 12), ('var_cam', 2), ('planner', 'NoMove'), ('gaze_method', 'Owl'), ('motion_profile', 'RVO'),
    ('max_flight_time', 5), ('drone_max_speed', 20), ('drone_view_depth', 60), ('dt', 0.2)])
def test_a_row_that_differs_in_what_the_batch_shares_is_refused_by_name(pkg, field, value):
    env, table = _env(pkg)
    bad = list(table)
    bad[3] = _changed(table[3], **{field: value})
    with pytest.raises(ValueError, match=rf'episode 3: {field} = .*per stream'):
        env.stream_episodes(episodes=bad)


def test_the_other_refusals(pkg, oracle):
    from drone2d_amd import runner, vec_env
    import stream_backend as SB
    env, table = _env(pkg, M=6)
    # the number of targets
    bad = list(table)
    bad[2] = _changed(table[2], target_list=[(40, 40), (250, 250)])
    with pytest.raises(ValueError, match='episode 2: target_list has 2 targets.*per stream'):
        env.stream_episodes(episodes=bad)
    # the derived cfg: the Kalman archive bounds take agent_radius
    bad = list(table)
    bad[1] = _changed(table[1], agent_radius=10)
    with pytest.raises(ValueError, match=r'episode 1: agent_radius = 10 .*d2d_cfg\.kf_lo_x.*per stream'):
        env.stream_episodes(episodes=bad)
    # map ids numpy cannot seed with: per row now
    for m in (-1, 2 ** 32, 1.5):
        bad = list(table)
        bad[3] = _changed(table[3], map_id=m)
        with pytest.raises(ValueError, match=r'episode 3: map_id .*2\*\*32'):
            env.stream_episodes(episodes=bad)
    ok = list(table)
    ok[3] = _changed(table[3], map_id=2 ** 32 - 1, agent_max_speed=20)      # the last seed, and a speed of its own: both per episode
    assert env._episode_table(ok)['map_id'][3] == 2 ** 32 - 1 and env._episode_table(ok)['env_par'][3, A.WE_SPEED] == 20
    # the first rows are the envs as constructed
    with pytest.raises(ValueError, match='episode 0: map_id .* is not that of env 0 as constructed'):
        env.stream_episodes(episodes=table[:0:-1])
    swapped = [table[0], _changed(table[1], init_position=(250, 250))] + table[2:]
    with pytest.raises(ValueError, match='episode 1: env_par .* is not that of env 1 as constructed'):
        env.stream_episodes(episodes=swapped)
    env2 = TM.table_stream_of(table[0], table, 2, redraw_agents=True).env
    env2.redraw_agents = False
    with pytest.raises(ValueError, match='episode 0: env_par .* as constructed'):
        env2.stream_episodes(episodes=table)
    # a row that is neither a Params nor a triple; a count that contradicts the table
    with pytest.raises(ValueError, match='episode 1: a row is a Params or a'):
        env.stream_episodes(episodes=[table[0], (1, 2)])
    with pytest.raises(ValueError, match='num_episodes 3 with a table of 6'):
        env.stream_episodes(3, episodes=table)
    # a backend without the assignment from a table; host-built worlds
    b = SB.backend_for_params(pkg_with_defaults(table[0]))
    old = b.attach(vec_env.VecDrone2DEnv(table[0], 2, backend=b, worlds='device', planner='Primitive', device_plugins=True, gaze='Oxford'))
    with pytest.raises(NotImplementedError, match='d2d_worlds_table.h.*build_worlds_of'):
        old.stream_episodes(episodes=table)
    b = TM.backend_for_params(pkg_with_defaults(table[0]))
    host = b.attach(vec_env.VecDrone2DEnv(table[0], 2, backend=b, planner='Primitive', device_plugins=True, gaze='Oxford'))
    with pytest.raises(NotImplementedError, match="worlds='device'"):
        host.stream_episodes(episodes=table)
    # the existing refusals hold for a table: a stream runs once
    xs = TM.table_stream_of(table[0], table, 2)
    xs.run()
    with pytest.raises(RuntimeError, match='streamed episodes already'):
        xs.env.stream_episodes(episodes=table)
    with pytest.raises(TypeError, match='episodes='):
        runner.EpisodeStream(table[0], 4, 2, episodes=table, backend=b)
    # the consecutive form is what it was: the map ids of one Params, through d2d_stream_assign
    calls = []
    xs = SB.stream_of(table[0], 3, 2)
    real = xs.env.backend.stream_assign
    xs.env.backend.stream_assign = lambda *a: (calls.append(a[2]), real(*a))[1]
    xs.run()
    assert calls and set(calls) == {5}


# ---------------------------------------------------------------------------------------------------------------- the study
def test_study_grid_is_the_scripts(pkg):
    from drone2d_amd import runner
    pairs = runner.study_pairs()
    axis = [40, 250, 460]
    assert len(pairs) == 72 and all(s != t for s, t in pairs)
    assert pairs == [(s, t) for s, t in product(product(axis, axis), product(axis, axis)) if s != t]
    assert pairs[0] == ((40, 40), (40, 250)) and pairs[-1] == ((460, 460), (460, 250))
    cells = list(runner.ValidationStudy('speed').cells())
    assert len(cells) == 27                                      # (3 agent numbers x 3 sizes) x 3 drone speeds, 360 episodes each: the script's 9720
    assert [c[0] for c in cells] == [(n, r, d, 'Primitive', 'Oxford') for n in (10, 20, 30) for r in (5, 10, 15) for d in (20, 40, 60)]
    for cell, p, table in cells:
        assert len(table) == 360 and p is table[0]
        assert [q.map_id for q in table] == [m for m in range(5) for _ in range(72)]
        assert [(q.init_position, q.target_list[0]) for q in table[72:144]] == pairs
        assert all(q.init_position != q.target_list[0] and len(q.target_list) == 1 for q in table)
        assert {(q.agent_number, q.agent_radius, q.agent_max_speed, q.drone_max_speed, q.planner, q.gaze_method) for q in table} == \
            {(cell[0], cell[1], 40, cell[2], 'Primitive', 'Oxford')}
    assert sum(len(t) for _, _, t in cells) // 360 == 27 and ('MPC' not in {c[0][3] for c in cells}) and 'MPC' in runner.ValidationStudy.__doc__
    size = list(runner.ValidationStudy('size').cells())
    assert [c[0] for c in size] == [(n, v, d, 'Jerk_Primitive', 'NoControl') for n in (10, 20, 30) for v in (20, 40, 60) for d in (20, 40, 60)]
    assert {(q.agent_radius, q.agent_max_speed) for q in size[4][2]} == {(-1, 40)}
    assert runner.ValidationStudy.KINDS['speed']['redraw'] and not runner.ValidationStudy.KINDS['size']['redraw']
    with pytest.raises(ValueError, match="'speed' or 'size'"):
        runner.ValidationStudy('shape')


def test_study_runs_a_cell_with_the_scripts_columns(pkg):
    """one small cell of each kind over the CPU backends: the 'speed' rows carry -1 and the redrawn worlds, the 'size' rows are
    experiment.py's"""
    from drone2d_amd import runner
    for kind, speed in (('speed', -1), ('size', 20)):
        study = runner.ValidationStudy(kind, agent_numbers=(3,), drone_max_speeds=(40,), map_ids=(1,), max_flight_time=2)
        cell, p, table = next(study.cells())
        table = table[:5]
        xs = TM.table_stream_of(p, table, 2, redraw_agents=study.spec['redraw'], agent_speed=study.spec['agent_speed'])
        rows = xs.run(refill_every=8)
        assert SM_same(rows, TM.rows_of_worlds(p, table, study.spec['redraw'], study.spec['agent_speed']))
        assert [r[7] for r in rows] == [speed] * 5 and [r[10] for r in rows] == [(40, 40)] * 5
        assert [r[11] for r in rows] == [t for _, t in runner.study_pairs()[:5]]
        assert len(runner.CSV_COLUMNS) == len(rows[0])


# ---------------------------------------------------------------------------------------------------------------- the model
def test_assign_table_model_is_the_assign_model_on_consecutive_ids():
    rs = np.random.RandomState(7)
    for B, M, cursor in ((5, 3, 3), (5, 5, 5), (5, 12, 5), (5, 12, 11), (5, 12, 12), (1030, 1500, 1030), (1030, 1040, 1036), (1, 4, 1)):
        for pattern in ('none', 'all', 'alternating', 'random'):
            done = {'none': np.zeros(B, bool), 'all': np.ones(B, bool), 'alternating': np.arange(B) % 2 == 0, 'random': rs.rand(B) < 0.4}[pattern]
            flags = rs.randint(0, 3, size=(B, 4)).astype(np.uint8)
            flags[:, A.F_DONE] = done
            slot0 = rs.permutation(max(B, cursor))[:B].astype(np.int32)
            slot0[rs.rand(B) < 0.1] = -1
            T, map_id0 = 2, 1000
            ep_map_id = (map_id0 + np.arange(M)).astype(np.uint32)
            ep_par, ep_tgt = rs.rand(M, A.WORLDS_ENV_F), rs.rand(M, T, 2)
            a = dict(slot=slot0.copy(), map_id=np.full(B, 77, np.uint32), refill=np.full(B, 9, np.uint8), counts=np.array([cursor, 5], np.int64))
            b = {k: v.copy() for k, v in a.items()}
            par0, tgt0 = rs.rand(B, A.WORLDS_ENV_F), rs.rand(B, T, 2)
            par, tgt = par0.copy(), tgt0.copy()
            SM.assign(flags, a['slot'], a['map_id'], a['refill'], a['counts'], M, map_id0)
            TM.assign_table(flags, b['slot'], b['map_id'], par, tgt, b['refill'], b['counts'], ep_map_id, ep_par, ep_tgt)
            for k in a:
                assert np.array_equal(a[k], b[k]), (B, M, cursor, pattern, k)
            got = b['refill'] == 1
            assert np.array_equal(par[got], ep_par[b['slot'][got]]) and np.array_equal(tgt[got], ep_tgt[b['slot'][got]])
            assert np.array_equal(par[~got], par0[~got]) and np.array_equal(tgt[~got], tgt0[~got])
            h = SM.harvested(flags, slot0)
            assert b['counts'][1] == 5 + h.sum() and b['counts'][0] == min(cursor + h.sum(), M)
            assert (b['slot'][h & ~got] == -1).all() and got.sum() == min(h.sum(), M - cursor)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_against_the_binder():
    from test_episode_stream_cpu import DECL, Recorder, argtypes_of
    declared = dict(re.findall(DECL, HEADER, re.M))
    assert sorted(declared) == sorted('d2d_' + n for n in A.TABLE_ENTRY_POINTS) == ['d2d_stream_assign_table']
    bound = A.bind_worlds_table(Recorder())
    fn = bound['stream_assign_table']
    assert fn.argtypes == argtypes_of(declared['d2d_stream_assign_table']) and fn.restype is C.c_int
    assert not set(bound) & set(A.bind_worlds_stream(Recorder())) and not set(bound) & set(A.bind_worlds(Recorder()))
    worlds = open(os.path.join(ROOT, 'include', 'd2d_worlds.h')).read()
    assert int(re.search(r'#define\s+D2D_WE_REDRAW\s+(\d+)', worlds).group(1)) == A.WE_REDRAW == 7 < A.WORLDS_ENV_F == 8
    assert 'D2D_WORLDS_VERSION 1' in worlds and 'D2D_WORLDS_VERSION 1' not in HEADER and A.D2D_WORLDS_VERSION == 1
    assert C.sizeof(A.WorldSpec) == 14 * 4 + 2 * 8 + 8 * 8


def test_a_library_without_the_symbol_loads_and_announces_none():
    from test_episode_stream_cpu import Recorder

    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_stream_assign_table':
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    assert A.bind_worlds_table(Old()) == {} and sorted(A.bind_worlds_stream(Old())) == sorted(A.STREAM_ENTRY_POINTS)
    hb = _lib.HipBackend.__new__(_lib.HipBackend)
    hb.sfn = A.bind_worlds_stream(Old())
    assert hb.supports_episode_stream is True and hb.supports_episode_table is False
    z = torch.zeros((2, 1, 2), dtype=torch.float64)
    with pytest.raises(_lib.D2DError, match='d2d_worlds_table.h'):
        hb.stream_assign_table(z, z, z, z, z, z, z, z, z, z)
    hb.sfn.update(A.bind_worlds_table(Recorder()))
    assert hb.supports_episode_table is True


def test_the_built_library_exports_it_and_refuses_bad_arguments_without_a_gpu(pkg):
    lib, wfn = _lib.load_worlds_library()
    fn = A.bind_worlds_table(lib)['stream_assign_table']
    one, err = C.c_void_p(8), wfn['last_error']          # never dereferenced: every call below is refused first
    assert wfn['version']() == 1
    assert fn(one, 2, 4, 0, one, one, one, one, one, one, one, one, one, None) == -1 and b'T >= 1' in err()
    assert fn(one, 2, A.STREAM_MAX_EPISODES + 1, 1, one, one, one, one, one, one, one, one, one, None) == -1 and b'MAX_EPISODES' in err()
    assert fn(one, 2, 4, 1, one, one, one, one, one, None, one, one, one, None) == -1 and b'a pointer is NULL' in err()
    assert fn(one, 2, 4, 1, one, None, one, one, one, one, one, one, one, None) == -1 and b'table pointer' in err()
    assert fn(None, 0, 4, 1, None, None, None, None, None, None, None, None, None, None) == 0
    # d2d_worlds_launch_shape: the redraw spends no LDS, so the shape is the parent's
    from drone2d_amd import vec_env
    for redraw in (False, True):
        inp = vec_env.world_inputs([pkg.Params(agent_number=70)], map_ids=range(3), redraw=redraw)
        out = (C.c_int32 * 2)()
        assert wfn['launch_shape'](C.byref(vec_env.world_spec(inp, 0, lambda n: 8)), C.byref(out)) == 0
        assert tuple(out) == (1, 8 * 4 * 70 + 4 * (8 + 624))
