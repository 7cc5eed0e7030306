"""include/d2d_rvo.h against its ctypes binding (drone2d_amd._abi), and the host side's refusals around motion_profile='RVO'."""
import ctypes as C
import os
import re

import pytest

from drone2d_amd import _abi as A
from drone2d_amd import _lib, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_rvo.h')).read()


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def test_every_entry_point_is_bound_with_the_header_s_arguments():
    kinds = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}
    lib = Recorder()
    bound = A.bind_rvo(lib)
    declared = re.findall(r'^(?:int|const char \*)\s*(d2d_rvo_\w+)\(([^;]*)\);', TEXT, re.M)
    assert sorted(n for n, _ in declared) == ['d2d_rvo_agents_step', 'd2d_rvo_last_error', 'd2d_rvo_velocity', 'd2d_rvo_version']
    assert sorted('d2d_rvo_' + k for k in bound) == sorted(n for n, _ in declared)
    for name, args in declared:
        args = args.replace('\n', ' ').strip()
        want = [] if args == 'void' else [C.c_void_p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        fn = bound[name[len('d2d_rvo_'):]]
        assert fn.argtypes == want, name
        assert fn.restype is (C.c_char_p if name.endswith('last_error') else C.c_int), name
    assert len(bound['velocity'].argtypes) == 8 and len(bound['agents_step'].argtypes) == 9


def test_version_and_limits_are_the_header_s():
    define = lambda n: int(re.search(r'#define\s+' + n + r'\s+(\w+)', TEXT).group(1), 0)   # noqa: E731
    assert define('D2D_RVO_VERSION') == A.D2D_RVO_VERSION == 1
    assert define('D2D_RVO_MAX_CONES') == A.RVO_MAX_CONES >= 171 and define('D2D_RVO_MAX_ELEMS') == A.RVO_MAX_ELEMS
    assert _lib._LIBRARIES['libd2d_rvo.so'][0] is A.bind_rvo and _lib.RVO_LIB_PATH.endswith(os.path.join('csrc', 'rvo', 'libd2d_rvo.so'))
    assert _lib.HipBackend.supports_rvo is True and callable(_lib.HipBackend.rvo_velocity) and callable(_lib.HipBackend.rvo_agents_step)
    assert callable(_lib.load_rvo_library)


def test_a_library_without_a_symbol_is_refused():
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_rvo_agents_step':
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    with pytest.raises(AttributeError):
        A.bind_rvo(Old())


def rvo_params(pkg, **kw):
    return pkg.Params(**dict(dict(planner='NoMove', motion_profile='RVO', agent_number=5, agent_radius=10, agent_max_speed=20, map_id=1), **kw))


def test_the_oracle_backend_is_refused_by_name(pkg, oracle):
    with pytest.raises(NotImplementedError, match='RVO') as e:
        vec_env.VecDrone2DEnv(rvo_params(pkg), 2, backend=oracle)
    assert 'oracle' in str(e.value)
    from drone2d_amd import env as envmod
    with pytest.raises(NotImplementedError, match='RVO'):
        envmod.Drone2DEnv2(rvo_params(pkg), backend=oracle)
    vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', agent_number=5, map_id=1), 2, backend=oracle).step(0.0)   # CVM: as before


def test_an_unknown_profile_is_a_value_error(pkg, oracle):
    with pytest.raises(ValueError, match='motion_profile'):
        vec_env.VecDrone2DEnv(rvo_params(pkg, motion_profile='ORCA'), 2, backend=oracle)


@pytest.mark.parametrize('kw', [dict(agent_max_speed=0), dict(agent_radius=-1)])
def test_parameters_the_reference_cannot_run_are_refused(pkg, oracle, kw):
    from rvo_backend import OracleRvoBackend
    for backend in (oracle, OracleRvoBackend()):
        with pytest.raises(NotImplementedError, match='RVO'):
            vec_env.VecDrone2DEnv(rvo_params(pkg, **kw), 2, backend=backend)


def test_closed_loop_under_rvo_raises(pkg):
    from drone2d_amd import runner
    from rvo_backend import OracleRvoBackend
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', motion_profile='RVO', agent_number=5, agent_radius=10, agent_max_speed=20,
                   drone_max_speed=40, map_id=1)
    env = vec_env.VecDrone2DEnv(p, 2, backend=OracleRvoBackend(), planner='Primitive', device_plugins=True, gaze='Oxford')
    with pytest.raises(NotImplementedError, match='RVO') as e:
        env.closed_loop(3)
    assert 'step()' in str(e.value) and 'Experiment' in str(e.value)
    with pytest.raises(NotImplementedError, match='RVO'):
        class Untouched:
            """the refusal comes before any world is built or any backend is asked for anything"""
            def __getattr__(self, name):
                raise AssertionError('backend touched: ' + name)
        runner.ExperimentBatch(p, 2, device='cpu', backend=Untouched())


def test_the_rvo_fields_of_a_batch_of_no_envs(pkg):
    """VecDrone2DEnv(..., 0, worlds='device') allocates a state of no envs: the pillars' shape comes from the parameters then"""
    import numpy as np
    from drone2d_amd import host_init, state
    for P in (0, 3):
        st = state.BatchState(host_init.derive_cfg(rvo_params(pkg, pillar_number=P), B=0, N=5, T=1), 'cpu')
        st.init_rvo(5, np.zeros((0, 0, 3)), P)
        assert tuple(st.pillars.shape) == (0, P, 3) and tuple(st.agent_vel.shape) == tuple(st.agent_vel_out.shape) == (0, 2, 5)
        assert st.clone_world().agent_vel is not st.agent_vel


def test_hand_built_worlds_without_pillars_still_run_the_constant_velocity_model(pkg, oracle):
    """worlds assembled from state tensors (tests/test_gpu_vs_oracle.py::_worlds) carry no 'obstacles': only RVO reads them"""
    p = pkg.Params(planner='NoMove', agent_number=5, map_id=1)
    worlds = [{k: v for k, v in w.items() if k != 'obstacles'} for w in vec_env.build_worlds(p, 2)]
    env = vec_env.VecDrone2DEnv(p, 2, backend=oracle, worlds=worlds)
    env.step(0.0)
    assert not env.rvo and 'pillars' not in env.state.t
