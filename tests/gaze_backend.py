"""Test-side backend for whole Jerk_Primitive episodes without a GPU: tests/jerk_backend.OracleJerkBackend (the CPU oracle for the
stages of include/d2d.h, the host build of the planner) plus the two entry points of include/d2d_gaze.h through the host build of
csrc/gaze/d2d_gaze.h (tests/csrc/gaze_host.c, which test_gaze_host_build.py holds against the host policies bit for bit).  Test
infrastructure: the product package never imports this."""
import ctypes as C
import os
import tempfile

import host_build
from drone2d_amd import _abi as A
from jerk_backend import OracleJerkBackend

_HOST = None


def host_library(tmpdir=None):
    global _HOST
    if _HOST is None:
        lib = host_build.shared('gaze_host.c', tmpdir or tempfile.mkdtemp(prefix='gaze_host_'), 'libgazehost.so',
                                include=os.path.join(host_build.CSRC, 'gaze'))
        V, I, D = C.c_void_p, C.c_int32, C.c_double
        lib.gaze_host_act.argtypes = [C.POINTER(A.GazeCall)]
        lib.gaze_host_reset.argtypes = [V, V, I, I]
        lib.gaze_host_mod360.argtypes, lib.gaze_host_mod360.restype = [D], D
        lib.gaze_host_lookahead.argtypes, lib.gaze_host_lookahead.restype = [D] * 5, D
        lib.gaze_host_offsets.argtypes = [V]
        _HOST = lib
    return _HOST


class OracleGazeBackend(OracleJerkBackend):
    name = 'oracle+jerk_host+gaze_host'
    supports_step_gaze = True

    def gaze_act(self, call):
        rc = host_library().gaze_host_act(C.byref(call))
        assert rc == 0, rc

    def gaze_reset(self, owl_state, mask=None, mask_stride=1):
        rc = host_library().gaze_host_reset(owl_state.data_ptr(), None if mask is None else mask.data_ptr(), int(mask_stride),
                                            owl_state.shape[0])
        assert rc == 0, rc
