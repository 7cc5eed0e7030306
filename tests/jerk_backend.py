"""Test-side backend for the Jerk_Primitive planner without a GPU: the CPU oracle for every stage of include/d2d.h plus the two entry
points of include/d2d_jerk.h through the host build of csrc/jerk/d2d_jerk.h (tests/csrc/jerk_host.c, which test_jerk_host_build.py
holds against the Python model bit for bit).  Test infrastructure: the product package never imports this."""
import ctypes as C
import os
import tempfile

import host_build
from drone2d_amd import _abi as A
from oracle_lib import OracleBackend

_HOST = None


def host_library():
    global _HOST
    if _HOST is None:
        lib = host_build.shared('jerk_host.c', tempfile.mkdtemp(prefix='jerk_host_'), 'libjerkhost.so',
                                include=os.path.join(host_build.CSRC, 'jerk'))
        V, I = C.c_void_p, C.c_int32
        lib.jerk_host_plan.argtypes = [C.POINTER(A.JerkCall), V]
        lib.jerk_host_reset.argtypes = [V, V, V, V, I, I, I]
        _HOST = lib
    return _HOST


class OracleJerkBackend(OracleBackend):
    name = 'oracle+jerk_host'
    supports_jerk = True

    def jerk_plan(self, call):
        import torch
        work = torch.zeros(5 * max(call.N, 1), dtype=torch.float64)
        rc = host_library().jerk_host_plan(C.byref(call), work.data_ptr())
        assert rc == 0, rc

    def jerk_reset(self, trk_radius, trk_prev, trk_radius0, mask=None, mask_stride=1):
        B, N = trk_radius.shape
        host_library().jerk_host_reset(trk_radius.data_ptr(), trk_prev.data_ptr(), trk_radius0.data_ptr(),
                                       None if mask is None else mask.data_ptr(), int(mask_stride), B, N)
