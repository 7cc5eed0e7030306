"""Test-side backends for action streams without a GPU (VecDrone2DEnv.action_stream): the stream backends of tests/stream_backend.py
with the two launches of include/d2d_worlds_turn.h restated in numpy -- d2d_stream_restore applies the packed item array to host
memory, byte range by byte range, and d2d_stream_explored is the count of stream_model.records.  `turn_model` is the whole turn
(harvest -> assign -> build -> restore -> resets) statement by statement, for the test that compares it with ActionStream's own.
Test infrastructure: the product package never imports this."""
import numpy as np

import stream_backend as SB
import table_model as TM
import stream_model as SM
from drone2d_amd import _abi as A


def restore_model(items_ptr, n_items, refill):
    """d2d_stream_restore over host memory: every item for every slot whose refill byte is set"""
    items = (A.RestoreItem * max(n_items, 1)).from_address(items_ptr)
    for k in range(n_items):
        it = items[k]
        if it.bytes <= 0 or it.kind not in (A.RESTORE_ZERO, A.RESTORE_COPY):
            continue
        for e in np.nonzero(np.asarray(refill))[0]:
            dst = SM.at(it.dst + int(e) * it.dst_stride + it.dst_off, (it.bytes,), np.uint8)
            dst[:] = 0 if it.kind == A.RESTORE_ZERO else SM.at(it.src + int(e) * it.src_stride + it.src_off, (it.bytes,), np.uint8)


class _Turn:
    supports_action_stream = True

    def stream_restore(self, items, n_items, refill):
        assert items.dtype.is_floating_point is False and items.numel() >= n_items * 64
        restore_model(items.data_ptr(), n_items, refill.numpy())

    def stream_explored(self, cfg, st, cells):
        from drone2d_amd import runner
        cells.copy_(cells.new_tensor(runner.batch_records(self.env)[:, A.STREAM_R_DMAP]))


class TurnPrimitiveBackend(_Turn, SB.StreamPrimitiveBackend):
    name = SB.StreamPrimitiveBackend.name + '+turn'


class TurnJerkBackend(_Turn, SB.StreamJerkBackend):
    name = SB.StreamJerkBackend.name + '+turn'


class TurnTablePrimitiveBackend(_Turn, TM.TablePrimitiveBackend):
    name = TM.TablePrimitiveBackend.name + '+turn'


class TurnTableJerkBackend(_Turn, TM.TableJerkBackend):
    name = TM.TableJerkBackend.name + '+turn'


def backend_for_params(params, table=False):
    """`table`: with the assignment from an episode table and a world build that reads each slot's own row (tests/table_model.py)"""
    jerk = params.planner == 'Jerk_Primitive'
    cls = (TurnTableJerkBackend if jerk else TurnTablePrimitiveBackend) if table else (TurnJerkBackend if jerk else TurnPrimitiveBackend)
    return cls().of(params)


def env_of(params, slots, backend=None, **kw):
    """VecDrone2DEnv of `params` with device worlds and the caller's gaze on a fresh turn backend, attached"""
    from drone2d_amd import vec_env
    backend = backend or backend_for_params(params)
    kw.setdefault('worlds', 'device')
    kw.setdefault('gaze', 'external')
    env = vec_env.VecDrone2DEnv(params, slots, device='cpu', backend=backend, planner=params.planner, device_plugins=True, **kw)
    return backend.attach(env)


TAB = np.linspace(-1, 1, 16)


def policy(episode, steps):
    """a = tab[(5 * episode + 3 * steps) % 16]: a deterministic action that depends on the episode and its step alone, so that an
    episode's record cannot depend on the slot or the schedule"""
    import torch
    tab = torch.as_tensor(TAB, device=episode.device)
    return tab[(5 * episode.long() + 3 * steps.long()) % 16]
