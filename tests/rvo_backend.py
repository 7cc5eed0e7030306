"""Test-side backend for the RVO motion profile without a GPU: the CPU oracle for every stage of include/d2d.h plus the two entry
points of include/d2d_rvo.h through the host build of csrc/rvo/d2d_rvo.h (tests/csrc/rvo_host.c, which test_rvo_host_build.py holds
against the Python model bit for bit).  Test infrastructure: the product package never imports this."""
import ctypes as C
import os
import tempfile

import host_build
from oracle_lib import OracleBackend

_HOST = None


def host_library():
    global _HOST
    if _HOST is None:
        lib = host_build.shared('rvo_host.c', tempfile.mkdtemp(prefix='rvo_host_'), 'librvohost.so', include=os.path.join(host_build.CSRC, 'rvo'))
        V, I, D = C.c_void_p, C.c_int32, C.c_double
        lib.rvo_host_velocity.argtypes = [V, V, V, I, I, I, V, V]
        lib.rvo_host_agents_step.argtypes = [V, V, D, D, D, D, I, I]
        _HOST = lib
    return _HOST


class OracleRvoBackend(OracleBackend):
    name = 'oracle+rvo_host'
    supports_rvo = True

    def rvo_velocity(self, agents, vel, pillars, vel_out):
        import torch
        B, _, N = agents.shape
        P = pillars.shape[1]
        work = torch.zeros(6 * max(N - 1 + P, 1), dtype=torch.float64)
        assert all(t.is_contiguous() for t in (agents, vel, pillars, vel_out)) and vel_out.data_ptr() != vel.data_ptr()
        rc = host_library().rvo_host_velocity(agents.data_ptr(), vel.data_ptr(), pillars.data_ptr() if P else None, B, N, P,
                                              vel_out.data_ptr(), work.data_ptr())
        assert rc == 0, rc

    def rvo_agents_step(self, agents, vel, W_px, H_px, scale, dt):
        B, _, N = agents.shape
        host_library().rvo_host_agents_step(agents.data_ptr(), vel.data_ptr(), float(W_px), float(H_px), float(scale), float(dt), B, N)
