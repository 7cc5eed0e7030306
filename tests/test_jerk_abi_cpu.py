"""include/d2d_jerk.h against its ctypes binding (drone2d_amd._abi), and the host side's refusals around planner='Jerk_Primitive'."""
import ctypes as C
import os
import re

import pytest

from drone2d_amd import _abi as A
from drone2d_amd import _lib, planners, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_jerk.h')).read()
KINDS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def test_every_entry_point_is_bound_with_the_header_s_arguments():
    bound = A.bind_jerk(Recorder())
    declared = re.findall(r'^(?:int|const char \*)\s*(d2d_jerk_\w+)\(([^;]*)\);', TEXT, re.M)
    assert sorted(n for n, _ in declared) == ['d2d_jerk_last_error', 'd2d_jerk_plan', 'd2d_jerk_reset', 'd2d_jerk_version']
    assert sorted('d2d_jerk_' + k for k in bound) == sorted(n for n, _ in declared)
    for name, args in declared:
        args = args.replace('\n', ' ').strip()
        want = [] if args == 'void' else [C.POINTER(A.JerkCall) if 'd2d_jerk_call' in a else C.c_void_p if '*' in a else KINDS[a.split()[0]]
                                          for a in args.split(',')]
        fn = bound[name[len('d2d_jerk_'):]]
        assert fn.argtypes == want, name
        assert fn.restype is (C.c_char_p if name.endswith('last_error') else C.c_int), name


def test_the_call_struct_is_the_header_s_field_for_field():
    body = re.search(r'typedef struct d2d_jerk_call \{(.*?)\} d2d_jerk_call;', TEXT, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip() for n in decl.split(',')]
        head = names[0].rsplit(None, 1)
        kind, names[0] = head[0], head[1]
        for n in names:
            ptr = '*' in kind or n.startswith('*')
            fields.append((n.lstrip('*'), C.c_void_p if ptr else KINDS[kind.replace('const', '').strip()]))
    assert fields == list(A.JerkCall._fields_)
    assert [n for n, t in fields if t is C.c_void_p] == list(A.JERK_CALL_POINTERS)


def test_version_and_limits_are_the_header_s():
    define = lambda n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', TEXT).group(1), 0)   # noqa: E731
    assert define('D2D_JERK_VERSION') == A.D2D_JERK_VERSION == 1
    for name in ('NTHETA', 'PATTERNS', 'MAX_S', 'MAX_N', 'TH_F', 'TT_F', 'STAT_TIE', 'STAT_UNKNOWN', 'STAT_SHIFT'):
        assert define('D2D_JERK_' + name) == getattr(A, 'JERK_' + name), name
    assert A.JERK_MAX_S == 128 and A.JERK_MAX_N >= 172                                       # BASELINE config 3: 172 agents
    assert _lib._LIBRARIES['libd2d_jerk.so'][0] is A.bind_jerk and _lib.JERK_LIB_PATH.endswith(os.path.join('csrc', 'jerk', 'libd2d_jerk.so'))
    assert _lib.HipBackend.supports_jerk is True and callable(_lib.HipBackend.jerk_plan) and callable(_lib.HipBackend.jerk_reset)
    assert callable(_lib.load_jerk_library)


def test_a_library_without_a_symbol_is_refused():
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_jerk_reset':
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    with pytest.raises(AttributeError):
        A.bind_jerk(Old())


def test_sizes_the_device_cannot_take_are_refused_on_the_host(pkg):
    """S > 128 (the same check the library answers with -4: tests/test_jerk_host_build.py), and more trackers than the wave's LDS
    holds; N == 0 is accepted and passes NULL tracker pointers"""
    from drone2d_amd import host_init, jerk_plugin, state
    with pytest.raises(ValueError, match='at most 128'):
        jerk_plugin.primitive_tables(2, 0.1)
    p = pkg.Params(planner='Jerk_Primitive', agent_number=0)
    st = state.BatchState(host_init.derive_cfg(p, B=2, N=0, T=1), 'cpu')
    js = jerk_plugin.JerkState(p, st.cfg, 'cpu', None)
    call = js.call(st)
    assert call.N == 0 and call.S == 9 and not call.active and not call.kf and not call.trk_radius and not call.trk_prev
    assert call.th_tab and call.tt_tab and call.tie_perm and call.tie_eq and call.wp and call.choice and call.stat and call.dmap
    big = state.BatchState(host_init.derive_cfg(p, B=1, N=A.JERK_MAX_N + 1, T=1), 'cpu')
    with pytest.raises(ValueError, match='at most 1024'):
        jerk_plugin.JerkState(p, big.cfg, 'cpu', None)
    with pytest.raises(ValueError, match='tie table'):
        jerk_plugin.JerkState(p, st.cfg, 'cpu', None, tie=(js.tie_np[0][:10], js.tie_np[1][:10]))


def test_without_tables_the_library_refuses(pkg):
    """NULL tables and outputs are -1 in d2d_jerk_plan; the host loop has no such check, so this is read off the source"""
    src = open(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'jerk', 'd2d_jerk.hip')).read()
    for text in ('a table pointer is NULL', 'an output pointer is NULL', 'a state pointer is NULL', 'a tracker pointer is NULL'):
        assert text in src
    assert re.search(r'c->S > D2D_JERK_MAX_S\) return failf\(-4', src) and re.search(r'c->N > D2D_JERK_MAX_N\) return failf\(-4', src)


@pytest.fixture
def device_jerk():
    """registers the device Jerk_Primitive and always takes it out again"""
    planners.enable_device_jerk()
    try:
        yield
    finally:
        planners.enable_device_jerk(False)


def test_planner_list_is_unchanged_around_enable_device_jerk():
    before = dict(planners.planner_list)
    assert set(before) == {'Primitive', 'NoMove'}
    planners.enable_device_jerk()
    try:
        assert planners.planner_list['Jerk_Primitive'] is planners.Jerk_Primitive and planners.Jerk_Primitive.on_device
    finally:
        planners.enable_device_jerk(False)
    assert dict(planners.planner_list) == before
    planners.enable_device_jerk(False)                                  # taking it out twice is harmless
    assert dict(planners.planner_list) == before

    class Theirs:
        pass
    planners.register_planner('Jerk_Primitive', Theirs)                 # somebody else's class under the name is not ours to remove
    try:
        planners.enable_device_jerk(False)
        assert planners.planner_list['Jerk_Primitive'] is Theirs
    finally:
        del planners.planner_list['Jerk_Primitive']
    assert dict(planners.planner_list) == before


def jerk_params(pkg, **kw):
    return pkg.Params(**dict(dict(planner='Jerk_Primitive', gaze_method='NoControl', agent_number=3, map_id=1), **kw))


def test_the_oracle_backend_is_refused_by_name(pkg, oracle):
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        vec_env.VecDrone2DEnv(jerk_params(pkg), 2, backend=oracle, planner='Jerk_Primitive', device_plugins=True)
    assert 'oracle' in str(e.value) and 'HIP backend' in str(e.value)
    # without device plugins the name is an external planner, as before: the caller supplies the plans
    env = vec_env.VecDrone2DEnv(jerk_params(pkg), 2, backend=oracle, planner='Jerk_Primitive')
    assert env.planner_mode == A.PLANNER_EXTERNAL and env.jerk is None


@pytest.mark.parametrize('gaze', ['Oxford', 'LookGoal', 'Owl', 'LookAhead'])
def test_gaze_stages_of_the_other_library_are_refused_with_this_planner(pkg, gaze):
    from jerk_backend import OracleJerkBackend
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        vec_env.VecDrone2DEnv(jerk_params(pkg), 2, backend=OracleJerkBackend(), planner='Jerk_Primitive', device_plugins=True, gaze=gaze)
    assert gaze in str(e.value) and 'Rotating' in str(e.value)


def test_closed_loop_and_experiment_batch_refuse_and_say_what_to_use(pkg):
    from drone2d_amd import runner
    from jerk_backend import OracleJerkBackend
    env = vec_env.VecDrone2DEnv(jerk_params(pkg), 2, backend=OracleJerkBackend(), planner='Jerk_Primitive', device_plugins=True)
    assert env.cfg.planner_mode == A.PLANNER_EXTERNAL
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        env.closed_loop(3)
    assert 'step()' in str(e.value) and 'runner.Experiment' in str(e.value) and 'libd2d_jerk.so' in str(e.value)
    with pytest.raises(NotImplementedError, match='Jerk_Primitive') as e:
        class Untouched:
            """the refusal comes before any world is built or any backend is asked for anything"""
            def __getattr__(self, name):
                raise AssertionError('backend touched: ' + name)
        runner.ExperimentBatch(jerk_params(pkg), 2, device='cpu', backend=Untouched())
    assert 'step()' in str(e.value) and 'runner.Experiment' in str(e.value)


def test_the_refusal_for_other_planner_names_is_unchanged(pkg, oracle):
    with pytest.raises(NotImplementedError) as e:
        vec_env.VecDrone2DEnv(pkg.Params(planner='MPC'), 2, backend=oracle, planner='MPC', device_plugins=True, gaze='Oxford')
    assert str(e.value) == ("device plugins: planner 'MPC' / gaze 'Oxford' "
                            '(device: Primitive, NoMove / Oxford, LookAhead, LookGoal, Owl, Rotating, NoControl)')
    from drone2d_amd import runner
    with pytest.raises(NotImplementedError, match='ExperimentBatch runs the device plugins'):
        runner.ExperimentBatch(pkg.Params(planner='MPC'), 2, device='cpu', backend=oracle)


def test_device_jerk_with_the_device_oxford_gaze_is_refused_in_the_facade(pkg, device_jerk):
    from drone2d_amd import env as envmod
    from jerk_backend import OracleJerkBackend
    with pytest.raises(NotImplementedError, match='Oxford'):
        envmod.Drone2DEnv2(jerk_params(pkg, gaze_method='Oxford'), backend=OracleJerkBackend())
