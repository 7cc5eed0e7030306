"""The launches of include/d2d_worlds_stream.h restated in numpy, for tests/stream_backend.py (whole streams without a GPU) and
for test_gpu_episode_stream.py (the kernels against this model).  Harvest is the record runner.batch_rows makes its tuples of, assign
is a loop in slot order, and the masked build is host_init.init_world loaded into the slot.  Test infrastructure."""
import copy
import ctypes as C

import numpy as np

from drone2d_amd import _abi as A

SENTINEL = -7          # what a test prefills `rows` with: the row of an episode that was not harvested must keep it


def records(counters, flags, dmap_logical):
    """[B, 8]: the numbers of runner.batch_rows, statement for statement (runner.batch_records), from numpy arrays; dmap_logical is
    [B, W, H] as the reference indexes it"""
    c, f = np.asarray(counters), np.asarray(flags)
    disc = (np.asarray(dmap_logical) != 0).reshape(len(c), -1).sum(1)
    out = np.zeros((len(c), A.STREAM_ROW_F), dtype=np.int64)
    out[:, [A.STREAM_R_STEPS, A.STREAM_R_SM, A.STREAM_R_BUF_N, A.STREAM_R_BUF_TS]] = c[:, [A.C_STEPS, A.C_SM, A.C_BUF_N, A.C_BUF_TS]]
    out[:, A.STREAM_R_FLAG0:A.STREAM_R_FLAG0 + 3] = f[:, :3]
    out[:, A.STREAM_R_DMAP] = disc
    return out


def harvested(flags, slot_episode):
    return (np.asarray(flags)[:, A.F_DONE] != 0) & (np.asarray(slot_episode) >= 0)


def harvest(rec, flags, slot_episode, rows):
    """rows[slot_episode[e]] = rec[e] for every slot that is done and not retired; `rows` in place"""
    for e in np.nonzero(harvested(flags, slot_episode))[0]:
        rows[int(slot_episode[e])] = rec[e]


def assign(flags, slot_episode, map_id, refill, counts, M, map_id0):
    """d2d_stream_assign as a loop in slot order; slot_episode, map_id (uint32), refill and counts = [cursor, finished] in place"""
    h = harvested(flags, slot_episode)
    cursor = int(counts[0])
    for e in range(len(h)):
        refill[e] = 0
        if not h[e]:
            continue
        if cursor < M:
            slot_episode[e] = cursor
            map_id[e] = (int(map_id0) + cursor) & 0xffffffff
            refill[e] = 1
            cursor += 1
        else:
            slot_episode[e] = -1
        counts[1] += 1
    counts[0] = cursor


def at(ptr, shape, dtype):
    """the array of `shape` that starts at address `ptr` (host memory), writable"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if not ptr or n == 0:
        return np.zeros(shape, dtype=dtype)
    return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)


def world_views(spec, st):
    """numpy views of everything d2d_worlds_build writes, behind the host pointers of a d2d_world_spec and a d2d_state"""
    B, N, P, T, W, H, tile = spec.B, spec.N, spec.P, spec.T, spec.W, spec.H, spec.grid_tile
    G = (-(-W // tile)) * (-(-H // tile)) * tile * tile if tile else W * H
    f64, i32, u8 = np.float64, np.int32, np.uint8
    v = dict(agents=at(st.agents, (B, A.AF, N), f64), agent_unit=at(st.agent_unit, (B, N), i32), dyn_prev=at(st.dyn_prev, (B, N, 3), i32),
             gt=at(st.gt, (B, G), u8), dmap=at(st.dmap, (B, G), u8), drone=at(st.drone, (B, A.DF), f64), target=at(st.target, (B, 2), f64),
             targets=at(st.targets, (B, T, 2), f64), counters=at(st.counters, (B, A.CF), i32), active=at(st.active, (B, N), u8),
             kf=at(st.kf, (B, N, A.KF), f64), kf_len=at(st.kf_len, (B, N), i32),
             tracker_radius=at(spec.tracker_radius, (B, N), f64), obstacles=at(spec.obstacles, (B, P, 3), i32),
             status=at(spec.status, (B,), i32), map_id=at(spec.map_id, (B,), np.uint32))
    if st.rng:
        v['rng'] = at(st.rng, (B, A.RNG_WORDS), np.uint32)
    if st.flags:
        v['flags'] = at(st.flags, (B, 4), u8)
    return v


def world_of(params, map_id):
    from drone2d_amd import host_init
    from drone2d_amd.params import with_defaults
    p = copy.copy(with_defaults(params))
    p.map_id = int(map_id)
    return host_init.init_world(p)


def load_world(v, e, w, grid_tile=0, flags=False):
    """host_init.init_world dict `w` (None: a world that hit max_attempts) into slot e of world_views `v`, as d2d_worlds_build leaves
    an env; `flags`: as d2d_worlds_build_masked, which writes the slot's flags too"""
    from drone2d_amd import state
    ok = w is not None
    for name in ('agents', 'agent_unit', 'dyn_prev', 'drone', 'target', 'targets', 'counters', 'tracker_radius', 'obstacles'):
        v[name][e] = np.asarray(w[name]).reshape(v[name][e].shape) if ok else 0
    for name in ('gt', 'dmap'):
        g = np.asarray(w[name]) if ok else None
        v[name][e] = 0 if g is None else (state.tile_grid(g, grid_tile).numpy() if grid_tile else g.reshape(-1))
    v['active'][e] = 0
    v['kf_len'][e] = 1 if ok else 0
    v['kf'][e] = 0
    if ok:
        for i, x in ((0, 1.0), (5, 1.0), (10, 10.0), (15, 10.0)):
            v['kf'][e][:, 4 + i] = x
    if 'rng' in v:
        v['rng'][e] = np.asarray(w['rng'], dtype=np.uint32) if ok else 0
    v['status'][e] = A.WORLD_OK if ok else A.WORLD_CAP
    if flags and 'flags' in v:
        v['flags'][e] = 0 if ok else [0, 0, 0, 1]
