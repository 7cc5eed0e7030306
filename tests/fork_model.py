"""numpy model of d2d_fork_slots (include/d2d_fork.h) over byte arrays: the definition, statement by statement, with none of the
kernel's partition into workgroups, units and ends.  An item is (dst, dst_base, dst_stride, src, src_base, src_stride, bytes) over
two flat uint8 arrays (the same array twice for a launch in place).  Also the handmade cases the host program
(tests/csrc/fork_host_main.c) and the GPU test run, their fill patterns and the digest the host program prints.
Test infrastructure: the product package never imports this."""
import numpy as np

LEFT, COPIED, REFUSED = 0, 1, 2
MAX_ITEMS = 64


def decide(src_of, B_src, in_place):
    """status [B_dst] uint8 from src_of alone"""
    src_of = np.asarray(src_of, dtype=np.int64)
    status = np.zeros(len(src_of), dtype=np.uint8)
    for e, s in enumerate(src_of):
        if s < 0:
            status[e] = LEFT
        elif s >= B_src:
            status[e] = REFUSED
        elif not in_place:
            status[e] = COPIED
        elif s == e:
            status[e] = LEFT
        else:
            status[e] = COPIED if (src_of[s] < 0 or src_of[s] == s) else REFUSED
    return status


def fork_slots(items, src_of, B_src, in_place, status):
    """the launch: `status` is overwritten, and row e of every item's dst becomes row src_of[e] of its src where status[e] is
    COPIED.  A source row is never a destination row of the same launch (in place the rule sees to it), so the order is free"""
    if len(items) > MAX_ITEMS:
        raise ValueError('d2d_fork_slots: 0 <= n_items <= D2D_FORK_MAX_ITEMS (64)')
    if in_place and B_src != len(src_of):
        raise ValueError('d2d_fork_slots: in place the source is the destination, B_src == B_dst')
    status[:] = decide(src_of, B_src, in_place)
    for dst, d0, dstride, src, s0, sstride, n in items:
        if n <= 0:
            continue
        for e in np.nonzero(status == COPIED)[0]:
            s = int(src_of[e])
            dst[d0 + e * dstride:d0 + e * dstride + n] = src[s0 + s * sstride:s0 + s * sstride + n].copy()


# ---- the handmade sets: GPU test 1 (between two batches) and 2 (in place), shared with the host program ----
ROWS = (1, 3, 4, 7, 16, 17, 64, 4099)
BASES = (0, 1, 4, 8)
BETWEEN = dict(B_dst=5, B_src=3, src_of=[2, -1, 0, 3, 2], in_place=0)
IN_PLACE = dict(B_dst=6, B_src=6, src_of=[0, 0, -1, 2, 5, 1], in_place=1)


def strides(n, k):
    """(dst_stride, src_stride) of item k with rows of n bytes: both differ from n and from each other, and item by item they
    change the alignment of row e against row s (so all three units, 16, 4 and 1 byte, are taken)"""
    return n + (5, 16, 4, 12)[k % 4], n + (11, 32, 8, 3)[k % 4]


def case_items(set_, rows=ROWS, bases=BASES):
    """[(bytes, dst_base, src_base, dst_stride, src_stride)] of a handmade set, one item per (row size, base offset): in place the
    source is the destination"""
    out = []
    for n in rows:
        for b in bases:
            k = len(out)
            ds, ss = strides(n, k)
            sb = bases[(bases.index(b) + k // len(bases)) % len(bases)]
            out.append((n, b, b if set_['in_place'] else sb, ds, ds if set_['in_place'] else ss))
    return out


def fill(size, seed):
    """the bytes a buffer holds before the launch (poison between the rows included): position and seed alone"""
    i = np.arange(size, dtype=np.uint64)
    return ((i * np.uint64(7 + 2 * seed) + np.uint64(seed) + (i >> np.uint64(8))) & np.uint64(0xff)).astype(np.uint8)


def extent(base, stride, n, B):
    """bytes of a buffer whose last row ends with it"""
    return base + stride * (B - 1) + n if B else base


def run_case(set_, item, index):
    """(dst bytes after the launch, status) of one item of a handmade set by the model"""
    n, db, sb, ds, ss = item
    B_dst, B_src = set_['B_dst'], set_['B_src']
    dst = fill(extent(db, ds, n, B_dst), 2 * index + 1)
    src = dst if set_['in_place'] else fill(extent(sb, ss, n, B_src), 2 * index + 2)
    status = np.full(B_dst, 0xee, dtype=np.uint8)
    fork_slots([(dst, db, ds, src, sb, ss, n)], set_['src_of'], B_src, set_['in_place'], status)
    return dst, status


def digest(*arrays):
    """a position-weighted sum modulo 2**64 over the arrays' bytes in order, sum (byte + 1) * (position + 1) * 0x9e3779b97f4a7c15:
    what the host program prints per case"""
    b = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]).astype(np.uint64)
    w = (np.arange(len(b), dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9e3779b97f4a7c15)
    with np.errstate(over='ignore'):
        return int(((b + np.uint64(1)) * w).sum(dtype=np.uint64))
