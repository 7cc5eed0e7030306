"""The selection rule of include/d2d_capture.h (d2d_capture_select) restated in Python, slot by slot, for tests/test_capture_cpu.py,
tests/capture_backend.py and tests/test_gpu_capture.py.  Test infrastructure: the product never imports this."""
import numpy as np

STATIC, DYNAMIC, DEAD_LOCK, FREEZING, GOAL, OTHER = range(1, 7)
NAMES = ('static', 'dynamic', 'dead_lock', 'freezing', 'goal', 'other')
F_COLLISION, F_DEADLOCK, F_FREEZING, F_DONE = 0, 1, 2, 3
C_STEPS, C_SM, SM_GOAL_REACHED = 0, 2, 1
ALL = (1 << 6) - 1


def mask(*names):
    return sum(1 << NAMES.index(n) for n in names)


def kind_of(flags4, counters8):
    """the first condition of the header's table that holds"""
    if flags4[F_COLLISION] == 1:
        return STATIC
    if flags4[F_COLLISION] == 2:
        return DYNAMIC
    if flags4[F_DEADLOCK]:
        return DEAD_LOCK
    if flags4[F_FREEZING]:
        return FREEZING
    if counters8[C_SM] == SM_GOAL_REACHED:
        return GOAL
    return OTHER


def row_kind(rec):
    """the kind of an episode from its stream record (D2D_STREAM_R_*: steps, sm, buf_n, buf_ts, flags[0..2], dmap)"""
    return kind_of([rec[4], rec[5], rec[6], 1], [rec[0], 0, rec[1]])


def select(flags, counters, drone, slot_episode, kinds, S, capacity, sel_slot, sel_dst, meta, pose, counts):
    """One call, in place: flags [B, 4], counters [B, 8], drone [B, 8], slot_episode [B] or None; sel_slot, sel_dst [S], meta
    [capacity, 4], pose [capacity, 3], counts [3] = taken, dropped, matched.  Returns the slots accepted"""
    B = len(flags)
    taken = int(counts[0])
    matches = accepted = 0
    took = []
    for e in range(B):
        ep = e if slot_episode is None else int(slot_episode[e])
        kind = kind_of(flags[e], counters[e])
        if not (flags[e][F_DONE] and ep >= 0 and counters[e][C_STEPS] > 0 and (kinds >> (kind - 1)) & 1):
            continue
        r = matches
        matches += 1
        if r < S and 0 <= taken and taken + r < capacity:
            sel_slot[r], sel_dst[r] = e, taken + r
            meta[taken + r] = (ep, kind, int(counters[e][C_STEPS]), e)
            pose[taken + r] = drone[e][:3]
            accepted += 1
            took.append(e)
    sel_slot[accepted:S] = -1
    sel_dst[accepted:S] = -1
    counts[0] += accepted
    counts[1] += matches - accepted
    counts[2] += matches
    return took


def fresh(S, capacity, taken=0):
    """(sel_slot, sel_dst, meta, pose, counts) poisoned, for a first call"""
    return (np.full(S, -7, np.int32), np.full(S, -7, np.int32), np.full((capacity, 4), -7, np.int32), np.full((capacity, 3), -7.0),
            np.array([taken, 0, 0], np.int64))
