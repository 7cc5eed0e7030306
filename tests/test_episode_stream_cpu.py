"""Episode streams without a GPU (VecDrone2DEnv.stream_episodes, runner.EpisodeStream) on the backends of tests/stream_backend.py:
the streamed rows are the batch runner's rows for the same map ids whatever the refill schedule, in all four cells of the planner x
motion-profile matrix; the edge counts, the refusals and the attempt cap; and include/d2d_worlds_stream.h against its ctypes binder."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import stream_backend as SB
from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'd2d_worlds_stream.h')).read()

COMMON = dict(agent_number=25, agent_radius=15, agent_max_speed=40, drone_max_speed=40, max_flight_time=4, map_id=3,
              target_list=[[90, 90]])
CELLS = {
    'Primitive-CVM': dict(planner='Primitive', gaze_method='Oxford'),
    'Primitive-RVO': dict(planner='Primitive', gaze_method='Oxford', motion_profile='RVO'),
    'Jerk-CVM': dict(planner='Jerk_Primitive', gaze_method='Owl'),
    'Jerk-RVO': dict(planner='Jerk_Primitive', gaze_method='LookAhead', motion_profile='RVO'),
}
M, SLOTS = 10, 3


def params_of(pkg, cell, **kw):
    return pkg.Params(**dict(dict(COMMON, **CELLS[cell]), **kw))


@functools.lru_cache(maxsize=None)
def batch_rows_of(cell):
    """the batch runner's rows for the M map ids, computed once per cell"""
    import drone2d_amd as pkg
    xb = SB.batch_of(params_of(pkg, cell), M)
    rows = xb.run()
    steps = [r[12] for r in rows]
    assert len(set(steps)) > 1, steps            # the episodes end at different steps, or the schedule would not matter
    assert max(steps) <= 4.0 + 0.1 + 1e-9
    return tuple(rows)


@pytest.mark.parametrize('cell', list(CELLS))
def test_stream_rows_are_the_batch_rows(pkg, cell):
    xs = SB.stream_of(params_of(pkg, cell), M, SLOTS)
    rows = xs.run()
    assert SB.same_rows(rows, batch_rows_of(cell)), (rows, batch_rows_of(cell))
    assert [r[3] for r in rows] == list(range(3, 3 + M)) and xs.build_failed == []
    assert xs.steps_run % 64 == 0 and xs.steps_run >= 64      # the default refill_every
    with pytest.raises(RuntimeError, match='has streamed'):
        xs.env.reset()


@pytest.mark.parametrize('refill_every', [1, 5, 16])
@pytest.mark.parametrize('cell', list(CELLS))
def test_rows_do_not_depend_on_the_refill_schedule(pkg, cell, refill_every):
    xs = SB.stream_of(params_of(pkg, cell), M, SLOTS)
    assert SB.same_rows(xs.run(refill_every=refill_every), batch_rows_of(cell))
    assert xs.steps_run % refill_every == 0


@pytest.mark.parametrize('m', [1, 2, 3])
def test_fewer_episodes_than_slots_and_as_many(pkg, m):
    cell = 'Jerk-CVM'
    xs = SB.stream_of(params_of(pkg, cell), m, SLOTS)
    assert SB.same_rows(xs.run(), batch_rows_of(cell)[:m])
    assert xs.records.shape == (m, A.STREAM_ROW_F)
    # a surplus slot was retired before the first step: nothing of it moved
    assert xs.env.state.counters[m:, A.C_STEPS].tolist() == [0] * (SLOTS - m)


def test_no_episodes(pkg):
    xs = SB.stream_of(params_of(pkg, 'Jerk-CVM'), 0, SLOTS)
    assert xs.run() == [] and xs.steps_run == 0


def test_refusals(pkg, oracle):
    from drone2d_amd import runner, vec_env
    from stepped_backend import SteppedOracleBackend
    p = params_of(pkg, 'Primitive-CVM')
    kw = dict(planner='Primitive', device_plugins=True, gaze='Oxford')
    # a backend that builds no worlds on the device / has no refill launches
    env = vec_env.VecDrone2DEnv(p, 2, backend=oracle, **kw)
    with pytest.raises(NotImplementedError, match='device world construction.*ExperimentBatch'):
        env.stream_episodes(4)
    half = SB.StreamPrimitiveBackend().of(p)
    half.supports_episode_stream = False
    env = half.attach(vec_env.VecDrone2DEnv(p, 2, backend=half, worlds='device', **kw))
    with pytest.raises(NotImplementedError, match='d2d_worlds_stream.h.*ExperimentBatch'):
        env.stream_episodes(4)
    # host-built worlds
    b = SB.StreamPrimitiveBackend().of(p)
    env = b.attach(vec_env.VecDrone2DEnv(p, 2, backend=b, **kw))
    with pytest.raises(NotImplementedError, match="worlds='device'"):
        env.stream_episodes(4)
    # the caller's noise rows
    q = params_of(pkg, 'Primitive-CVM', var_cam=2)
    b = SB.StreamPrimitiveBackend().of(q)
    env = b.attach(vec_env.VecDrone2DEnv(q, 2, backend=b, worlds='device', **kw))
    with pytest.raises(NotImplementedError, match='supports_device_noise'):
        env.stream_episodes(4)
    env.set_noise(np.zeros((2, env.N, 2)))
    with pytest.raises(NotImplementedError, match='set_noise'):
        env.stream_episodes(4)
    # map ids past numpy's seeds
    r = params_of(pkg, 'Primitive-CVM', map_id=2 ** 32 - 3)
    b = SB.StreamPrimitiveBackend().of(r)
    env = b.attach(vec_env.VecDrone2DEnv(r, 2, backend=b, worlds='device', **kw))
    with pytest.raises(ValueError, match=r'2\*\*32.*split'):
        env.stream_episodes(4)
    # a policy the device does not evaluate
    b = SB.StreamPrimitiveBackend().of(p)
    env = b.attach(vec_env.VecDrone2DEnv(p, 2, backend=b, worlds='device', planner='Primitive', device_plugins=True, gaze='external'))
    with pytest.raises(RuntimeError, match='gaze policy the device evaluates'):
        env.stream_episodes(4)
    # EpisodeStream keeps the batch runners' refusals
    with pytest.raises(NotImplementedError, match='ExperimentBatch runs the device plugins'):
        runner.EpisodeStream(pkg.Params(planner='Primitive', gaze_method='Nonesuch'), 4, 2, backend=SteppedOracleBackend())
    with pytest.raises(NotImplementedError, match='SteppedExperimentBatch: gaze_method'):
        runner.EpisodeStream(pkg.Params(planner='Jerk_Primitive', gaze_method='Nonesuch'), 4, 2, backend=SteppedOracleBackend())
    with pytest.raises(NotImplementedError, match='EpisodeStream: LookAhead needs a backend'):
        runner.EpisodeStream(params_of(pkg, 'Primitive-CVM', gaze_method='LookAhead'), 4, 2, backend=SteppedOracleBackend())
    with pytest.raises(RuntimeError, match=r'run\(\) first'):
        SB.stream_of(p, 2, 2).rows()


def test_a_stream_runs_once_and_only_on_envs_as_constructed(pkg):
    """after a stream every slot is retired and holds the last world that passed through it: a second run would harvest those as
    episodes 0 .. B - 1.  It is refused, as is a stream on an env that has been stepped, and an auto reset from the stale snapshot"""
    from drone2d_amd import vec_env
    p = params_of(pkg, 'Jerk-CVM')
    xs = SB.stream_of(p, 4, 2)
    rows = xs.run()
    with pytest.raises(RuntimeError, match='new EpisodeStream'):
        xs.run()
    assert SB.same_rows(xs.rows(), rows) and SB.same_rows(rows, batch_rows_of('Jerk-CVM')[:4])
    with pytest.raises(RuntimeError, match='streamed episodes already.*new VecDrone2DEnv / EpisodeStream'):
        xs.env.stream_episodes(4)
    # an env that has been stepped: refused until reset() puts the constructed worlds back
    b = SB.backend_for_params(p)
    env = b.attach(vec_env.VecDrone2DEnv(p, 2, backend=b, worlds='device', planner=p.planner, device_plugins=True, gaze=p.gaze_method))
    env.policy_step()
    with pytest.raises(RuntimeError, match='has been stepped.*new VecDrone2DEnv / EpisodeStream'):
        env.stream_episodes(4)
    env.reset()
    rec = env.stream_episodes(4).numpy()
    assert np.array_equal(rec, xs.records)
    # the persistent loop's auto reset restores the snapshot of the construction
    q = params_of(pkg, 'Primitive-CVM')
    xs = SB.stream_of(q, 3, 2)
    xs.run()
    with pytest.raises(RuntimeError, match=r'closed_loop\(auto_reset=True\).*streamed'):
        xs.env.closed_loop(1, auto_reset=True)


def test_batch_rows_is_made_of_the_records(pkg):
    """batch_rows is batch_records + record_row, and the model's record is batch_records"""
    import stream_model as SM
    from drone2d_amd import runner
    xb = SB.batch_of(params_of(pkg, 'Jerk-CVM'), 3)
    rows = xb.run()
    rec = runner.batch_records(xb.env)
    s = xb.env.state
    assert np.array_equal(rec, SM.records(s.counters.numpy(), s.flags.numpy(), s.dmap.numpy()))
    assert SB.same_rows(rows, [runner.record_row(xb.params, 3 + e, rec[e]) for e in range(3)])
    assert SB.same_rows(rows, batch_rows_of('Jerk-CVM')[:3])


def test_a_world_that_hits_max_attempts_is_marked_and_the_stream_goes_on(pkg):
    """max_attempts = 32 with 25 agents: a world whose first 32 candidates do not hold 25 free ones cannot be placed.  The first
    SLOTS episodes are the envs as constructed (the constructor's own cap); of the ones the stream builds, those the sequential
    host form of the construction marks as capped come back as rows of zeros, the others as the batch runner's rows"""
    cell, cap = 'Jerk-CVM', 32
    p = params_of(pkg, cell)
    capped = [k >= SLOTS and SB._capped(pkg, SB.backend_for_params(p).params, 3 + k, cap) for k in range(M)]
    assert any(capped) and not all(capped[SLOTS:]), capped
    xs = SB.stream_of(p, M, SLOTS)
    rows = xs.run(max_attempts=cap)
    assert xs.build_failed == [3 + k for k in range(M) if capped[k]]
    want = batch_rows_of(cell)
    for k in range(M):
        if capped[k]:
            assert not xs.records[k].any() and xs.records[k, A.STREAM_R_STEPS] == A.STREAM_BUILD_FAILED
            assert rows[k][3] == 3 + k and rows[k][12] == 0
        else:
            assert SB.same_rows([rows[k]], [want[k]]), k


# ---------------------------------------------------------------------------------------------------------------- the ABI
DECL = r'^int\s*(d2d_\w+)\(([^;]*)\);'
KINDS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'double': C.c_double}
STRUCTS = {'d2d_state': A.State, 'd2d_world_spec': A.WorldSpec}


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def argtypes_of(args):
    out = []
    for a in args.replace('\n', ' ').strip().split(','):
        words = a.replace('*', ' * ').split()
        if '*' in words:
            struct = STRUCTS.get(words[1] if words[0] == 'const' else words[0])
            out.append(C.POINTER(struct) if struct else C.c_void_p)
        else:
            out.append(KINDS[words[0]])
    return out


def test_the_header_against_the_binder():
    declared = dict(re.findall(DECL, HEADER, re.M))
    assert sorted(declared) == sorted('d2d_' + n for n in A.STREAM_ENTRY_POINTS) == ['d2d_stream_assign', 'd2d_stream_clear',
                                                                                  'd2d_stream_harvest', 'd2d_worlds_build_masked']
    bound = A.bind_worlds_stream(Recorder())
    for name, args in declared.items():
        fn = bound[name[len('d2d_'):]]
        assert fn.argtypes == argtypes_of(args), name
        assert fn.restype is C.c_int, name
    # the masked build takes d2d_worlds_build's arguments with `refill` in front of the stream
    pinned = A.bind_worlds(Recorder())
    m = list(bound['worlds_build_masked'].argtypes)
    assert m[:2] + m[3:] == list(pinned['build'].argtypes) and m[2] is C.c_void_p
    assert not set(bound) & set(pinned) and sorted(pinned) == ['build', 'last_error', 'launch_shape', 'version']
    define = lambda n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', HEADER).group(1), 0)   # noqa: E731
    for name in ('F_DONE', 'ROW_F', 'R_STEPS', 'R_SM', 'R_BUF_N', 'R_BUF_TS', 'R_FLAG0', 'R_DMAP', 'BUILD_FAILED', 'MAX_EPISODES'):
        assert define('D2D_STREAM_' + name) == getattr(A, 'STREAM_' + name), name
    assert A.STREAM_F_DONE == A.F_DONE == 3
    assert 'D2D_WORLDS_VERSION 1' not in HEADER and A.D2D_WORLDS_VERSION == 1
    assert _lib._LIBRARIES['libd2d_worlds.so'][0] is A.bind_worlds      # the stream functions are bound on the same loaded library


def test_a_library_without_the_stream_symbols_loads_and_announces_none():
    class Old(Recorder):
        def __getattr__(self, name):
            if name in ('d2d_' + n for n in A.STREAM_ENTRY_POINTS):
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    assert A.bind_worlds_stream(Old()) == {} and sorted(A.bind_worlds(Old())) == ['build', 'last_error', 'launch_shape', 'version']
    hb = _lib.HipBackend.__new__(_lib.HipBackend)
    hb.sfn = A.bind_worlds_stream(Old())
    assert hb.supports_episode_stream is False
    with pytest.raises(_lib.D2DError, match='d2d_worlds_stream.h'):
        z = torch.zeros(2, dtype=torch.int32)
        hb.stream_assign(z, 0, 0, z, z, z, z)
    hb.sfn = A.bind_worlds_stream(Recorder())
    assert hb.supports_episode_stream is True


def test_the_built_library_exports_them_and_refuses_bad_arguments_without_a_gpu(pkg):
    """bad arguments are refused before any launch, so this runs without a GPU"""
    from drone2d_amd import vec_env
    lib, wfn = _lib.load_worlds_library()
    fn = A.bind_worlds_stream(lib)
    assert sorted(fn) == sorted(A.STREAM_ENTRY_POINTS) and wfn['version']() == 1
    one, st = C.c_void_p(8), A.State()          # never dereferenced: every call below is refused first
    err = wfn['last_error']
    assert fn['stream_harvest'](C.byref(st), one, 2, 50, 50, 8, 4, one, None) == -1 and b'grid_tile' in err()
    assert fn['stream_harvest'](C.byref(st), one, 2, 50, 50, 0, A.STREAM_MAX_EPISODES + 1, one, None) == -1 and b'MAX_EPISODES' in err()
    assert fn['stream_harvest'](C.byref(st), one, 2, 50, 50, 0, 4, one, None) == -1 and b'NULL' in err()
    assert fn['stream_harvest'](C.byref(st), one, 0, 50, 50, 0, 4, one, None) == 0
    assert fn['stream_assign'](one, 2, 4, 2 ** 32 - 3, one, one, one, one, None) == -1 and b'2^32' in err()
    assert fn['stream_assign'](one, 2, 4, 0, one, one, None, one, None) == -1 and b'NULL' in err()
    assert fn['stream_assign'](None, 0, 4, 0, None, None, None, None, None) == 0
    inp = vec_env.world_inputs([pkg.Params(agent_number=10)], map_ids=range(1, 5))
    spec = vec_env.world_spec(inp, 0, lambda n: 8)
    assert fn['worlds_build_masked'](C.byref(spec), C.byref(st), None, None) == -1 and b'refill is NULL' in err()
    assert fn['worlds_build_masked'](C.byref(spec), C.byref(st), one, None) == -1 and b'world field' in err()
    spec.version += 1
    assert fn['worlds_build_masked'](C.byref(spec), C.byref(st), one, None) == -2
    assert fn['stream_clear'](one, 6, one, 2, None) == -1 and b'multiple of 4' in err()
    assert fn['stream_clear'](C.c_void_p(6), 8, one, 2, None) == -1 and b'aligned' in err()
    assert fn['stream_clear'](one, 8, None, 2, None) == -1 and b'NULL' in err()
    assert fn['stream_clear'](None, 8, None, 0, None) == 0 and fn['stream_clear'](one, 0, one, 2, None) == 0
