"""Test-side backends for slot forks without a GPU (VecDrone2DEnv.load_slots / fork / sibling, whatif.branch_terms): the launch of
include/d2d_fork.h done by tests/fork_model.py on the host memory behind the packed item array, mixed into the CPU stand-ins of the
other test modules.  One backend serves one env (the stand-ins read their env's tensors), so `sibling_of` gives the second env a
backend of its own.  Test infrastructure: the product package never imports this."""
import numpy as np

import action_stream_backend as AB
import fork_model as FM
import stream_model as SM
import tracks_backend as TB
from drone2d_amd import _abi as A
from jerk_live_backend import LiveJerkBackend
from stepped_backend import SteppedOracleBackend


def fork_model_launch(items_ptr, n_items, src_of, B_src, in_place, status):
    """d2d_fork_slots over host memory: the packed records become fork_model items over flat views of their buffers"""
    if n_items > A.FORK_MAX_ITEMS:
        raise ValueError('d2d_fork error -1: d2d_fork_slots: 0 <= n_items <= D2D_FORK_MAX_ITEMS (64)')
    recs = (A.ForkItem * max(n_items, 1)).from_address(items_ptr) if n_items else []
    B_dst, items = len(src_of), []
    for k in range(n_items):
        it = recs[k]
        if it.bytes <= 0:
            continue
        dst = SM.at(it.dst, (FM.extent(0, it.dst_stride, it.bytes, B_dst),), np.uint8)
        src = SM.at(it.src, (FM.extent(0, it.src_stride, it.bytes, B_src),), np.uint8)
        items.append((dst, 0, it.dst_stride, src, 0, it.src_stride, it.bytes))
    FM.fork_slots(items, src_of, B_src, in_place, status)


class _Fork:
    supports_fork = True
    fork_launches = 0

    def fork_slots(self, items, n_items, src_of, B_src, in_place, status):
        assert not items.dtype.is_floating_point and items.numel() >= n_items * 40
        self.fork_launches += 1
        fork_model_launch(items.data_ptr(), n_items, src_of.numpy(), int(B_src), int(bool(in_place)), status.numpy())


class ForkOracleBackend(_Fork, SteppedOracleBackend):
    name = SteppedOracleBackend.name + '+fork'


class ForkJerkBackend(_Fork, LiveJerkBackend):
    name = LiveJerkBackend.name + '+fork'


class ForkAllBackend(_Fork, TB.AllOracleBackend):
    """the four observation channels and the fork on one env"""
    name = TB.AllOracleBackend.name + '+fork'


class ForkTurnBackend(_Fork, AB.TurnPrimitiveBackend):
    """... with d2d_stream_explored, which whatif.branch_terms counts the discovered cells with"""
    name = AB.TurnPrimitiveBackend.name + '+fork'


class ForkTurnJerkBackend(_Fork, AB.TurnJerkBackend):
    name = AB.TurnJerkBackend.name + '+fork'


def backend_of(params, channels=False, turn=False):
    """a fresh backend for an env of `params`"""
    from drone2d_amd.params import with_defaults
    p = with_defaults(params)
    jerk = p.planner == 'Jerk_Primitive'
    if channels:
        b = ForkAllBackend()
        b.seen_view_range = p.drone_view_range
        return b
    if turn:
        return (ForkTurnJerkBackend if jerk else ForkTurnBackend)().of(p)
    return (ForkJerkBackend if jerk else ForkOracleBackend)()


def env_of(params, B, channels=False, turn=False, **kw):
    """VecDrone2DEnv of `params` on a fresh fork backend, attached"""
    from drone2d_amd import vec_env
    backend = backend_of(params, channels, turn)
    kw.setdefault('device_plugins', True)
    kw.setdefault('planner', params.planner)
    env = vec_env.VecDrone2DEnv(params, B, device='cpu', backend=backend, **kw)
    env._fork_backend_args = (params, channels, turn)
    return backend.attach(env)


def sibling_of(env, num_envs):
    """env.sibling(num_envs) on a backend of its own, attached"""
    backend = backend_of(*env._fork_backend_args)
    sib = env.sibling(num_envs, backend=backend)
    sib._fork_backend_args = env._fork_backend_args
    return backend.attach(sib)
