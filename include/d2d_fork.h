/*
 * d2d_fork.h — C ABI of the slot fork (libd2d_fork.so): whole per-slot rows of any number of per-slot buffers copied from a source
 * slot chosen per destination slot, in one launch -- between two batches (VecDrone2DEnv.load_slots) or inside one
 * (VecDrone2DEnv.fork).  It is what a what-if over gaze actions, a population step or a kept state needs: the state of a slot is some
 * forty tensors over nine holders, and this is the one place that copies a row of all of them.
 *
 * d2d_stream_restore (d2d_worlds_turn.h) puts ranges back from a sibling buffer of the SAME slot; this launch is the same list of
 * items with a source slot index per destination slot.
 *
 * Definition.  For every destination slot e < B_dst, with s = src_of[e]:
 *   s < 0                              status[e] = D2D_FORK_LEFT; nothing of slot e is read or written
 *   s >= B_src                         status[e] = D2D_FORK_REFUSED; nothing written
 *   in_place == 0                      status[e] = D2D_FORK_COPIED; for every item, bytes [dst + e * dst_stride, + bytes) become
 *                                      bytes [src + s * src_stride, + bytes)
 *   in_place != 0 (dst and src are the same buffers, B_src == B_dst)
 *     s == e                           D2D_FORK_LEFT
 *     src_of[s] < 0 || src_of[s] == s  D2D_FORK_COPIED, as above: the source slot is not written by this launch
 *     otherwise                        D2D_FORK_REFUSED: the source is itself a destination; nothing written for e
 * Nothing outside the named rows is written.  The in-place rule is decided from src_of alone, two loads per workgroup: a slot is
 * read only if no workgroup of the launch writes it, so the result does not depend on the order the workgroups run in and needs
 * neither atomics nor a second buffer.  status is written for every slot and read by nobody inside the call.
 *
 * Launch.  D2D_FORK_PARTS workgroups of one wave per destination slot (the shape of d2d_stream_restore).  An item of more than
 * D2D_FORK_SMALL_BYTES is cut into that many runs, one per workgroup; a smaller one belongs whole to workgroup (item index modulo the
 * parts).  The workgroups of a slot that is left or refused return behind their loads of src_of.  Rows are copied in 16-byte
 * accesses where the source and the destination address agree modulo 16, in 4-byte ones where they agree modulo 4 only, and in single
 * bytes at the two ends and for rows that agree in neither.
 *
 * Conventions as in d2d_tracks.h: plain C, the caller owns all memory, DEVICE pointers (the item array too: the argument list stays
 * small and a caller builds it once), asynchronous on the caller's stream, 0 or a negative error (-1 NULL pointer or bad argument, -3
 * HIP launch error, -4 a size the launch cannot hold) with a thread-local message and no launch.  The rows are the caller's to keep
 * inside their buffers: the library cannot look into device memory before a launch.  The library is separate from the others and
 * reports its own version.
 */
#ifndef D2D_FORK_H
#define D2D_FORK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_FORK_VERSION 1

typedef struct d2d_fork_item { /* one per-slot buffer: row e is bytes [base + e * stride, + bytes) */
  void *dst;
  const void *src;
  int64_t dst_stride, src_stride; /* bytes; the two buffers may have different slot counts, never different rows */
  int64_t bytes;                  /* of one row; any count, any alignment of base and stride; <= 0 copies nothing */
} d2d_fork_item;

#define D2D_FORK_MAX_ITEMS 64
#define D2D_FORK_PARTS 8            /* workgroups (of one wave) per destination slot */
#define D2D_FORK_SMALL_BYTES 4096   /* a row of at most this many bytes belongs to one workgroup */
#define D2D_FORK_LEFT 0    /* src_of[e] < 0 or (in place) src_of[e] == e: nothing of slot e is read or written */
#define D2D_FORK_COPIED 1
#define D2D_FORK_REFUSED 2 /* src_of[e] >= B_src; or in place and the source is itself a destination (above) */

int d2d_fork_version(void);
const char *d2d_fork_last_error(void);

/* B_dst, B_src >= 0 (B_dst == 0: nothing to do); 0 <= n_items <= D2D_FORK_MAX_ITEMS (0: status alone is written); in_place != 0
 * needs B_src == B_dst.  -4: B_dst * D2D_FORK_PARTS workgroups exceed the grid */
int d2d_fork_slots(const d2d_fork_item *items /* device */, int32_t n_items, const int32_t *src_of /* device [B_dst] */, int32_t B_dst,
                   int32_t B_src, int32_t in_place, uint8_t *status /* device [B_dst] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_FORK_H */
