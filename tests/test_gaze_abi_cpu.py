"""include/d2d_gaze.h against its ctypes binding (drone2d_amd._abi) and against the layouts of include/d2d.h it restates."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from drone2d_amd import _abi as A
from drone2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, 'include', 'd2d_gaze.h')).read()
D2D_H = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
KINDS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}


class Recorder:
    def __getattr__(self, name):
        fn = type('fn', (), {})()
        self.__dict__[name] = fn
        return fn


def define(name, text=TEXT):
    return int(re.search(r'#define\s+' + name + r'\s+(\w+)', text).group(1), 0)


def test_every_entry_point_is_bound_with_the_header_s_arguments():
    bound = A.bind_gaze(Recorder())
    declared = re.findall(r'^(?:int|const char \*)\s*(d2d_gaze_\w+)\(([^;]*)\);', TEXT, re.M)
    assert sorted(n for n, _ in declared) == ['d2d_gaze_act', 'd2d_gaze_last_error', 'd2d_gaze_reset', 'd2d_gaze_version']
    assert sorted('d2d_gaze_' + k for k in bound) == sorted(n for n, _ in declared)
    for name, args in declared:
        args = args.replace('\n', ' ').strip()
        want = [] if args == 'void' else [C.POINTER(A.GazeCall) if 'd2d_gaze_call' in a else C.c_void_p if '*' in a else KINDS[a.split()[0]]
                                          for a in args.split(',')]
        fn = bound[name[len('d2d_gaze_'):]]
        assert fn.argtypes == want, name
        assert fn.restype is (C.c_char_p if name.endswith('last_error') else C.c_int), name


def test_the_call_struct_is_the_header_s_field_for_field():
    body = re.search(r'typedef struct d2d_gaze_call \{(.*?)\} d2d_gaze_call;', TEXT, re.S).group(1)
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
    assert fields == list(A.GazeCall._fields_)
    assert [n for n, t in fields if t is C.c_void_p] == list(A.GAZE_CALL_POINTERS)


def test_version_limits_and_the_restated_layouts():
    assert define('D2D_GAZE_VERSION') == A.D2D_GAZE_VERSION == 1
    assert define('D2D_GAZE_K_LOOKAHEAD') == A.GAZE_K_LOOKAHEAD == define('D2D_GAZE_LOOKAHEAD', D2D_H)
    assert define('D2D_GAZE_K_OWL') == A.GAZE_K_OWL == define('D2D_GAZE_OWL', D2D_H)
    assert define('D2D_GAZE_MAX_N') == A.GAZE_MAX_N == 1024 and A.GAZE_MAX_N >= 172            # BASELINE config 3: 172 agents
    for mine, theirs, py in (('OWL_STATE_F', 'D2D_OWL_STATE_F', A.OWL_STATE_F), ('OWL_S_RATE', 'D2D_OWL_S_RATE', A.OWL_S_RATE),
                             ('OWL_S_LEFT', 'D2D_OWL_S_LEFT', A.OWL_S_LEFT), ('OWL_TAB_LEN', 'D2D_OWL_TAB_LEN', A.OWL_TAB_LEN)):
        assert define('D2D_GAZE_' + mine) == define(theirs, D2D_H) == py, mine


def test_the_library_is_registered_and_the_backend_says_so():
    assert _lib._LIBRARIES['libd2d_gaze.so'][0] is A.bind_gaze and _lib._LIBRARIES['libd2d_gaze.so'][2] == 'D2D_GAZE_VERSION'
    assert _lib._LIBRARIES['libd2d_gaze.so'][4] == 'gaze/build.sh'
    assert os.path.isfile(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'gaze', 'build.sh'))
    assert _lib.GAZE_LIB_PATH.endswith(os.path.join('csrc', 'gaze', 'libd2d_gaze.so'))
    assert _lib.HipBackend.supports_step_gaze is True and callable(_lib.HipBackend.gaze_act) and callable(_lib.HipBackend.gaze_reset)
    assert callable(_lib.load_gaze_library)


def test_a_library_without_a_symbol_is_refused():
    class Old(Recorder):
        def __getattr__(self, name):
            if name == 'd2d_gaze_reset':
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    with pytest.raises(AttributeError):
        A.bind_gaze(Old())


def test_sizeof_and_offsets_through_a_compiled_probe(tmp_path):
    """the gcc build of csrc/gaze/d2d_gaze.h: the struct's size, and the owl_tab offsets it restates from include/d2d.h"""
    import gaze_backend
    lib = gaze_backend.host_library(tmp_path)
    assert lib.gaze_host_call_bytes() == C.sizeof(A.GazeCall) and lib.gaze_host_version() == A.D2D_GAZE_VERSION
    out = np.zeros(32, np.int32)
    n = lib.gaze_host_offsets(out.ctypes.data)
    want = [A.OWL_T_RATE, A.OWL_T_RATE08, A.OWL_T_TURN, A.OWL_T_ACT, A.OWL_T_DIR, A.OWL_T_FOV, A.OWL_T_DEPTH, A.OWL_T_HOLD,
            A.OWL_TAB_LEN, A.OWL_STATE_F, A.OWL_S_RATE, A.OWL_S_LEFT, A.OWL_NRATE, A.OWL_NDIR, A.GAZE_MAX_N, A.GAZE_K_LOOKAHEAD,
            A.GAZE_K_OWL, A.F_DONE, A.DF, A.KF]
    assert out[:n].tolist() == want
    for name, v in zip(('RATE', 'RATE08', 'TURN', 'ACT', 'DIR', 'FOV', 'DEPTH', 'HOLD'), want):
        assert define('D2D_OWL_T_' + name, D2D_H) == v


def test_the_state_object_builds_the_call(pkg):
    """GazeState over a BatchState on the host: pointers, NULLs at N == 0, the done mask on request, sizes it refuses"""
    from drone2d_amd import gaze_plugin, host_init, state
    p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', agent_number=0)
    st = state.BatchState(host_init.derive_cfg(p, B=3, N=0, T=1), 'cpu')
    gs = gaze_plugin.GazeState(p, st.cfg, 'cpu', 'Owl')
    c = gs.call(st)
    assert (c.B, c.N, c.kind, c.reserved, c.dt, c.yaw_rate_max) == (3, 0, A.GAZE_K_OWL, 0, p.dt, p.drone_max_yaw_speed)
    assert not c.active and not c.kf and c.drone and c.target and c.flags and c.owl_state and c.owl_tab and c.action
    assert c.flags == st.t['flags'].data_ptr() and c.action == st.t['action'].data_ptr() and not gs.call(st, skip_done=False).flags
    assert gs.owl_state.shape == (3, A.OWL_STATE_F) and not gs.owl_state.any()
    la = gaze_plugin.GazeState(p, st.cfg, 'cpu', 'LookAhead')
    assert la.owl_state is None and la.call(st).kind == A.GAZE_K_LOOKAHEAD and not la.call(st).owl_tab
    with pytest.raises(ValueError, match='LookGoal'):
        gaze_plugin.GazeState(p, st.cfg, 'cpu', 'LookGoal')
    big = state.BatchState(host_init.derive_cfg(p, B=1, N=A.GAZE_MAX_N + 1, T=1), 'cpu')
    with pytest.raises(ValueError, match='at most 1024'):
        gaze_plugin.GazeState(p, big.cfg, 'cpu', 'Owl')


def test_the_library_refuses_bad_arguments_before_any_launch():
    """-1 / -4 come before the first hipLaunchKernelGGL of d2d_gaze_act: read off the source (test_gpu_gaze.py calls it)"""
    src = open(os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'gaze', 'd2d_gaze.hip')).read()
    body = src[src.index('int d2d_gaze_act('):]
    first_launch = body.index('hipLaunchKernelGGL')
    for text in ('B >= 1, N >= 0', 'return failf(-4', 'D2D_GAZE_K_LOOKAHEAD (%d) or D2D_GAZE_K_OWL (%d)'):
        assert 0 <= body.index(text) < first_launch, text
