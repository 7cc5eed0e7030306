"""Action streams on the device (VecDrone2DEnv.action_stream, include/d2d_worlds_turn.h): d2d_stream_restore alone over poisoned
buffers against a byte model, d2d_stream_explored against the logical grid in both layouts, and the stream itself -- its rows against a
reference batch in all four planner x motion-profile cells whatever the schedule, a refilled slot against a fresh env in every tensor,
the restore against _refill_rest, the terminal state, and the table form against stream_episodes().  Every comparison is exact.

The reference of the rows is a 12-env VecDrone2DEnv of the same map ids with gaze='external', every env stepped with a = policy(env,
step) and its record kept from the first step at which its done byte is set (action_stream_cases.reference_records).  Two things in
it are not the one-line step() loop one would write first.  The Primitive plugins' step() runs no plan stage, so their reference step
is perceive(), d2d_plan_stage, act().  And the stream's driver queues the turn itself (ActionStream.turn) in front of the policy: with
the turn left to step(), a fresh episode's first action is the one computed from the terminal state of the episode the slot played
before, and a record would depend on the slot and the schedule -- by construction, not by a fault."""

import numpy as np
import pytest
import torch

import action_stream_cases as AC
from drone2d_amd import _abi as A

pytestmark = pytest.mark.gpu


def _make(hip):
    def make(params, n, **kw):
        from drone2d_amd import vec_env
        kw.setdefault('worlds', 'device')
        kw.setdefault('gaze', 'external')
        return vec_env.VecDrone2DEnv(params, n, backend=hip, planner=params.planner, device_plugins=True, **kw)
    return make


def _records(items, dev):
    arr = (A.RestoreItem * max(len(items), 1))()
    for r, it in zip(arr, items):
        r.dst, r.src, r.dst_stride, r.src_stride, r.dst_off, r.src_off, r.bytes, r.kind, r.reserved = it
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(dev)


def test_restore_alone_writes_the_named_ranges_and_nothing_else(hip):
    """B = 70: a ZERO of 1089 bytes a slot at a base offset of 3 bytes (every slot starts unaligned, a few words and both ends), a ZERO
    of 153 600 bytes (cut over the slot's workgroups), a COPY of 40 bytes with src_stride != dst_stride and offsets that leave source
    and destination differently aligned.  The buffers are poisoned; the poison is intact outside the ranges and in every slot whose
    refill byte is 0.  Then n_items = 0, and B = 1."""
    B, dev = 70, hip.device
    rs = np.random.RandomState(20)
    mask = (rs.rand(B) < 0.5).astype(np.uint8)
    assert mask[:64].any() and not mask[:64].all() and mask[64:].any() and not mask[64:].all()
    sizes = dict(a=3 + B * 1089 + 5, b=B * 153616, c=B * 100, src=B * 77)
    host = {k: np.full(n, 0xA5, dtype=np.uint8) for k, n in sizes.items()}
    host['src'] = rs.randint(0, 256, size=sizes['src']).astype(np.uint8)
    buf = {k: torch.from_numpy(v.copy()).to(dev) for k, v in host.items()}
    ranges = [('a', None, 1089, 0, 3, 0, 1089, A.RESTORE_ZERO), ('b', None, 153616, 0, 8, 0, 153600, A.RESTORE_ZERO),
              ('c', 'src', 100, 77, 13, 5, 40, A.RESTORE_COPY)]
    items = _records([(buf[d].data_ptr(), buf[s].data_ptr() if s else None, ds, ss, do, so, n, kind, 0) for d, s, ds, ss, do, so, n, kind in ranges], dev)

    def model(refill, nslots):
        for d, s, ds, ss, do, so, n, kind in ranges:
            for e in np.nonzero(refill[:nslots])[0]:
                host[d][e * ds + do:e * ds + do + n] = 0 if kind == A.RESTORE_ZERO else host[s][e * ss + so:e * ss + so + n]

    def check(what):
        hip.sync()
        for k in host:
            assert np.array_equal(buf[k].cpu().numpy(), host[k]), (what, k)

    refill = torch.from_numpy(mask).to(dev)
    hip.stream_restore(items, 0, refill)                     # no items: nothing is written
    check('n_items = 0')
    one = torch.ones(1, dtype=torch.uint8, device=dev)
    hip.stream_restore(items, 3, one)                        # B = 1: slot 0 alone
    model(np.ones(1, dtype=np.uint8), 1)
    check('B = 1')
    assert (host['a'][:3] == 0xA5).all() and (host['a'][3:3 + 1089] == 0).all() and host['a'][3 + 1089] == 0xA5
    hip.stream_restore(items, 3, refill)
    model(mask, B)
    check('B = 70')
    assert (host['b'] == 0).sum() == 153600 * int(mask[1:].sum() + 1) and (host['c'] != 0xA5).sum() <= 40 * int(mask[1:].sum() + 1)
    hip.stream_restore(items, 3, torch.zeros(B, dtype=torch.uint8, device=dev))     # no slot: nothing is written
    check('no slot')


@pytest.mark.parametrize('W,H,layout', [(29, 31, 'rowmajor'), (40, 35, 'tiled')], ids=['29x31-rowmajor', '40x35-tiled'])
def test_explored_counts_the_cells_of_every_slot(pkg, hip, W, H, layout):
    """29 x 31 row-major: 899 bytes a slot, so every slot starts unaligned.  40 x 35 forced into the tiled layout: partial edge tiles,
    their padding bytes 0xFF beforehand -- cells are counted, not bytes"""
    from drone2d_amd import host_init, vec_env
    from drone2d_amd.params import with_defaults
    from drone2d_amd.state import BatchState, tile_grid
    B = 7
    p = with_defaults(pkg.Params(planner='NoMove', map_size=[10 * W, 10 * H], map_scale=10, agent_number=2))
    cfg = host_init.derive_cfg(p, B=B, N=2, T=1, grid_tile=vec_env._grid_tile(p, hip, layout))
    st = BatchState(cfg, hip.device)
    assert (cfg.grid_tile == 16) == (layout == 'tiled')
    rs = np.random.RandomState(W)
    logical = rs.randint(0, 256, size=(B, W, H)).astype(np.uint8)
    logical[rs.rand(B, W, H) < 0.45] = 0
    logical[3] = 0                                            # a slot with nothing discovered
    logical[5] = 200                                          # ... and one with everything
    if cfg.grid_tile:
        stored = tile_grid(torch.from_numpy(logical)).numpy().copy()
        padding = tile_grid(torch.ones((B, W, H), dtype=torch.uint8)).numpy() == 0
        assert padding.any() and stored.shape[1] == 3 * 3 * 256
        stored[padding] = 0xFF
    else:
        stored = logical.reshape(B, -1)
        assert stored.shape[1] == 899
    st.dmap.copy_(torch.from_numpy(stored).reshape(st.dmap.shape))
    cells = torch.full((B,), -3, dtype=torch.int32, device=hip.device)
    hip.stream_explored(cfg, st.struct(), cells)
    hip.sync()
    want = (logical != 0).reshape(B, -1).sum(1)
    assert cells.cpu().numpy().tolist() == want.tolist() and want[3] == 0 and want[5] == W * H
    assert torch.equal(st.logical('dmap').cpu(), torch.from_numpy(logical))


_reference = {}


def _reference_records(hip, pkg, cell):
    if cell not in _reference:
        _reference[cell] = AC.reference_records(_make(hip), AC.params_of(pkg, cell))
    return _reference[cell]


@pytest.mark.parametrize('cell', list(AC.CELLS))
def test_rows_do_not_depend_on_the_schedule_or_the_slot(pkg, hip, cell):
    """12 episodes over 5 slots at refill_every 1 and 3: the same rows, and those of the reference batch.  The worlds are not quiet:
    an episode ends by collision, another by freezing, and a slot is refilled twice"""
    p = AC.params_of(pkg, cell)
    want = _reference_records(hip, pkg, cell)
    print(cell, 'reference', want.tolist())
    assert (want[:, A.STREAM_R_FLAG0] != 0).any() and ((want[:, A.STREAM_R_FLAG0 + 2] != 0) | (want[:, A.STREAM_R_SM] == A.SM_GOAL_REACHED)).any()
    got = {}
    for every in (1, 3):
        got[every], calls, refills = AC.stream_rows(_make(hip), p, AC.SLOTS, AC.M, every)
        print(cell, 'every', every, 'calls', calls, 'refills', refills.tolist(), got[every].tolist())
        assert refills.max() >= 2 and refills.sum() == AC.M - AC.SLOTS
    assert np.array_equal(got[1], got[3])
    assert np.array_equal(got[1], want)


@pytest.mark.parametrize('m', [3, 5], ids=['M3-two-slots-retired', 'M5-as-many-as-slots'])
def test_fewer_episodes_than_slots_and_as_many(pkg, hip, m):
    cell = 'Jerk-CVM'
    rows, calls, refills = AC.stream_rows(_make(hip), AC.params_of(pkg, cell), AC.SLOTS, m, 1)
    assert np.array_equal(rows, _reference_records(hip, pkg, cell)[:m]) and refills.sum() == 0 and calls <= AC.MAX_STEPS + 1


@pytest.mark.parametrize('cell', ['Primitive-RVO', 'Jerk-RVO'])
def test_a_refilled_slot_is_a_fresh_env(pkg, hip, cell):
    AC.check_refilled_slot_is_fresh(_make(hip), pkg, cell)


@pytest.mark.parametrize('cell', ['Primitive-RVO', 'Jerk-RVO'])
def test_the_restore_is_refill_rest(pkg, hip, cell):
    """two identical envs (the static map's cell agents among theirs: the COPY items), stepped alike, get the same refill mask: one
    goes through _refill_rest(), the other through the item list and the masked resets.  Every tensor is equal afterwards"""
    from drone2d_amd import action_stream
    make = _make(hip)
    p = AC.params_of(pkg, cell, static_map='maps/obstacle_map.npy', agent_number=10)
    envs = [make(p, 6), make(p, 6)]
    assert envs[0].cfg.N > 10
    act = torch.linspace(-1, 1, 6, dtype=torch.float64, device=hip.device)
    for env in envs:
        for _ in range(3):
            AC.unmasked_step(env, act)
    refill = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=hip.device)
    envs[0]._refill_rest(refill)
    prev = torch.full((6,), 7, dtype=torch.int32, device=hip.device)
    listed = action_stream.restore_items(envs[1], prev)
    items, n = action_stream.pack_items(listed, hip.device)
    hip.stream_restore(items, n, refill)
    envs[1].reset_plugins(refill)
    hip.sync()
    assert prev.tolist() == [0, 7, 0, 0, 7, 0]
    for e in range(6):
        assert AC.differing(AC.tensors(envs[0], e), AC.tensors(envs[1], e)) == [], e
    vel = envs[1].state.agent_vel
    assert bool(vel[0, :, 10:].ne(0).any()) and not bool(vel[0, :, :10].ne(0).any()) and bool(envs[1].state.obs_local[1].ne(0).any())


@pytest.mark.parametrize('cell', ['Primitive-CVM', 'Jerk-RVO'])
def test_the_terminal_state_is_visible_until_the_next_call(pkg, hip, cell):
    AC.check_terminal_state(_make(hip), pkg, cell)


def test_the_table_form_against_the_device_gaze_stream(pkg, hip):
    from drone2d_amd import runner, vec_env
    AC.check_table_form(pkg, lambda p, table, slots: runner.EpisodeStream(p, episodes=table, slots=slots, backend=hip),
                        lambda p, slots, worlds: _make(hip)(p, slots, worlds=worlds),
                        lambda plist: vec_env.build_worlds_device_of(plist, backend=hip))
