"""Slot forks on the device (include/d2d_fork.h, libd2d_fork.so; VecDrone2DEnv.fork_items / load_slots / fork / sibling,
whatif.branch_terms).  Every comparison is exact equality.

  1  the launch alone over poisoned buffers, against the numpy model (tests/fork_model.py): rows of 1 .. 4099 bytes at base offsets 0, 1,
     4 and 8 in slices of a larger tensor, strides that differ from the rows, 5 <- 3 slots with a slot left and one out of range;
     with 0, 32 and D2D_FORK_MAX_ITEMS items, and one item more is an error return with a message
  2  in place: the refusal rule, and two launches from the same start give identical bytes
  3  twins (tests/fork_cases.py): a sibling loaded from an env stays bit-equal to it, item for item, over 25 more steps, in six cells
  4  fork in place, then diverge
  5  from a live action stream: the sibling follows the stream, and the stream's records are those of a stream nobody read
  6  whatif.branch_terms against twins built by hand
  7  completeness: every per-slot tensor reachable from the holders is an item or has its line in fork.EXCLUDED
"""
import numpy as np
import pytest
import torch

import fork_cases as FC
import fork_model as FM
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu
GUARD = 64             # poison behind every item's last row


def layout(set_, copies=1):
    """the items of a handmade set as regions of two flat buffers: [(bytes, dst offset, src offset, dst_stride, src_stride)], and the
    buffers' sizes.  A region starts at a multiple of 64 plus the item's base offset and ends with GUARD bytes of poison"""
    items, dn, sn = [], 0, 0
    for _ in range(copies):
        for n, db, sb, ds, ss in FM.case_items(set_):
            if set_['in_place']:
                items.append((n, dn + db, dn + db, ds, ds))
            else:
                items.append((n, dn + db, sn + sb, ds, ss))
                sn = -(-(sn + FM.extent(sb, ss, n, set_['B_src']) + GUARD) // 64) * 64
            dn = -(-(dn + FM.extent(db, ds, n, set_['B_dst']) + GUARD) // 64) * 64
    return items, dn, (dn if set_['in_place'] else sn)


def launch(hip, set_, items, dst, src, n_items=None):
    """d2d_fork_slots over the device buffers; returns the status bytes (prefilled with 0xee)"""
    n = len(items) if n_items is None else n_items
    arr = (A.ForkItem * max(len(items), 1))()
    for rec, (nb, do, so, ds, ss) in zip(arr, items):
        rec.dst, rec.src, rec.dst_stride, rec.src_stride, rec.bytes = dst.data_ptr() + do, src.data_ptr() + so, ds, ss, nb
    packed = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(hip.device)
    src_of = torch.tensor(set_['src_of'], dtype=torch.int32, device=hip.device)
    status = torch.full((set_['B_dst'],), 0xee, dtype=torch.uint8, device=hip.device)
    hip.fork_slots(packed, n, src_of, set_['B_src'], set_['in_place'], status)
    hip.sync()
    return status.cpu().numpy()


def modelled(set_, items, dst, src):
    status = np.full(set_['B_dst'], 0xee, dtype=np.uint8)
    FM.fork_slots([(dst, do, ds, src, so, ss, nb) for nb, do, so, ds, ss in items], set_['src_of'], set_['B_src'], set_['in_place'], status)
    return status


@pytest.mark.parametrize('copies, n_items', [(1, None), (1, 0), (2, None)])
def test_the_launch_alone_over_poisoned_buffers(hip, copies, n_items):
    set_ = FM.BETWEEN
    items, dn, sn = layout(set_, copies)
    assert len(items) == (A.FORK_MAX_ITEMS if copies == 2 else 32)
    dst0, src0 = FM.fill(dn, 1), FM.fill(sn, 2)
    dst, src = torch.from_numpy(dst0.copy()).to(hip.device), torch.from_numpy(src0.copy()).to(hip.device)
    status = launch(hip, set_, items, dst, src, n_items)
    want_dst = dst0.copy()
    want_status = modelled(set_, items if n_items is None else items[:n_items], want_dst, src0)
    assert status.tolist() == want_status.tolist() == [1, 0, 1, 2, 1]
    assert np.array_equal(dst.cpu().numpy(), want_dst)                 # result and every poison byte
    assert np.array_equal(src.cpu().numpy(), src0)
    assert (n_items == 0) == np.array_equal(want_dst, dst0)


def test_one_item_more_than_the_launch_takes_is_an_error_with_a_message(hip):
    from drone2d_amd import _lib
    set_ = FM.BETWEEN
    items, dn, sn = layout(set_, 3)
    dst, src = torch.from_numpy(FM.fill(dn, 1)).to(hip.device), torch.from_numpy(FM.fill(sn, 2)).to(hip.device)
    with pytest.raises(_lib.D2DError, match=r'd2d_fork error -1: d2d_fork_slots: 0 <= n_items <= D2D_FORK_MAX_ITEMS'):
        launch(hip, set_, items[:A.FORK_MAX_ITEMS + 1], dst, src)
    assert np.array_equal(dst.cpu().numpy(), FM.fill(dn, 1))            # no launch


def test_in_place_the_rule_and_the_order(hip):
    set_ = FM.IN_PLACE
    items, dn, _ = layout(set_)
    start = FM.fill(dn, 3)
    runs = []
    for _ in range(2):
        buf = torch.from_numpy(start.copy()).to(hip.device)
        status = launch(hip, set_, items, buf, buf)
        runs.append((buf.cpu().numpy(), status))
    want = start.copy()
    want_status = modelled(set_, items, want, want)
    # slots 1 and 3 are copied; 4 is refused (its source, slot 5, is written) and so is 5 (its source, slot 1, is written); 0 and 2 are left
    assert want_status.tolist() == [0, 1, 0, 1, 2, 2]
    for got, status in runs:
        assert status.tolist() == want_status.tolist() and np.array_equal(got, want)
    assert np.array_equal(runs[0][0], runs[1][0])
    assert not np.array_equal(want, start)


# ---------------------------------------------------------------------------------------------------- envs
def make_of(pkg, hip, cell, **more):
    from drone2d_amd import vec_env

    def make(B=FC.B_A):
        p = FC.params_of(pkg, cell)
        return vec_env.VecDrone2DEnv(p, B, backend=hip, planner=p.planner, device_plugins=True, **dict(FC.env_kw(cell), **more))
    return make


def sibling(env, n):
    return env.sibling(n)


@pytest.mark.parametrize('cell', list(FC.CELLS))
def test_twins(pkg, hip, cell):
    """Witnesses (tests/fork_cases.py WITNESS, chosen on the CPU stand-ins with tools/fork_cells.py): in every cell but jerk_rvo slot
    0 of A (map id 8) has run a plan search before the fork, tracks one agent at the fork (step 7) and is ended by the freezing rule at step 25;
    in jerk_rvo it is slot 1 (map id 1).  No cell lacked a witness below map id 64."""
    assert all(getattr(hip, flag, False) for flag in FC.CELLS[cell][2])

    def held(env):                             # the Owl cell forks while a decision is being held
        if cell == 'jerk_cvm_owl':
            assert bool((env.gaze_state.owl_state[:, A.OWL_S_LEFT] > 0).all())
        if cell == 'primitive_cvm_noise':
            assert env.device_noise and 'state.rng' in {n for n, _, _ in env.fork_items()}
    FC.twins(make_of(pkg, hip, cell), sibling, FC.WITNESS[cell], at_fork=held)


@pytest.mark.parametrize('cell', ['primitive_cvm', 'jerk_rvo'])
def test_fork_in_place_then_diverge(pkg, hip, cell):
    FC.in_place_case(make_of(pkg, hip, cell))


def test_from_a_live_action_stream(pkg, hip):
    from drone2d_amd import vec_env

    def make(p, B):
        return vec_env.VecDrone2DEnv(p, B, backend=hip, planner='Primitive', device_plugins=True, gaze='external', worlds='device')
    FC.stream_case(pkg, make, sibling)


def test_branch_terms(pkg, hip):
    got = FC.branch_case(make_of(pkg, hip, 'primitive_cvm'), sibling)
    assert all(v.device.type == 'cuda' for v in got.values())


@pytest.mark.parametrize('cell', ['primitive_cvm_channels', 'jerk_owl_rvo'])
def test_completeness(pkg, hip, cell):
    from drone2d_amd import vec_env
    if cell == 'jerk_owl_rvo':
        p = pkg.Params(planner='Jerk_Primitive', gaze_method='Owl', motion_profile='RVO', pillar_number=2, map_id=1, **FC._BASE)
        env = vec_env.VecDrone2DEnv(p, 3, backend=hip, planner='Jerk_Primitive', device_plugins=True, gaze='Owl')
    else:
        env = make_of(pkg, hip, cell)(3)
    names = FC.completeness(env)
    assert {'state.drone', 'state.kf'} <= names and len(names) >= (30 if cell == 'jerk_owl_rvo' else 50)
    env.lidar = {'ranges': torch.zeros(3, 8)}
    with pytest.raises(AssertionError, match='env.lidar'):
        FC.completeness(env)
