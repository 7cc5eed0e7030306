/*
 * d2d_worlds_turn.h — the two launches that make the turnover of d2d_worlds_stream.h cheap enough to queue at every step, for a
 * stream whose gaze actions come from the caller (libd2d_worlds.so; VecDrone2DEnv.action_stream, action_stream.ActionStream).
 *
 * The stream of d2d_worlds_stream.h reads `counts` back after every assignment and puts back the state outside the world with a
 * dozen masked fills and four or five d2d_stream_clear launches.  That is fine every 64 steps.  A learner steps the env itself and
 * wants a finished slot in a fresh world at its next step, so there the turn is queued unconditionally, nothing is read back, and
 *
 *   d2d_stream_restore    one launch puts back every per-slot range outside the world for the slots whose refill byte is set:
 *                         zeroes, or copies out of another per-slot buffer (the cell agents' velocities under RVO)
 *   d2d_stream_explored   one wave per slot counts the non-zero cells of the slot's dmap, as d2d_stream_harvest counts them, for
 *                         every slot: the per-step "cells discovered" a reward is made of
 *
 * d2d_stream_harvest, d2d_stream_assign / d2d_stream_assign_table, d2d_worlds_build_masked and the masked resets are used as they
 * are.  Additions to the library: D2D_WORLDS_VERSION does not change with them, and a caller looks them up as optional symbols.
 * Error codes and the thread-local message (d2d_worlds_last_error) are as in d2d_worlds.h.
 */
#ifndef D2D_WORLDS_TURN_H
#define D2D_WORLDS_TURN_H

#include <stdint.h>

#include "d2d_worlds_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_RESTORE_MAX_ITEMS 32
#define D2D_RESTORE_ZERO 0 /* bytes [dst + e * dst_stride + dst_off, .. + bytes) become 0 */
#define D2D_RESTORE_COPY 1 /* the same bytes become those at src + e * src_stride + src_off; the two ranges do not overlap */

/* One range of every refilled slot.  Strides, offsets and `bytes` are in bytes; any base alignment and any byte count: the
 * destination is written in whole words where its address allows and in single bytes at the two ends.  `src` is read only by
 * D2D_RESTORE_COPY.  An item with bytes <= 0 or an unknown kind writes nothing. */
typedef struct d2d_restore_item {
  void *dst;
  const void *src;
  int64_t dst_stride;
  int64_t src_stride;
  int64_t dst_off;
  int64_t src_off;
  int64_t bytes;
  int32_t kind;
  int32_t reserved; /* 0 */
} d2d_restore_item;

/* `items`: a DEVICE array of n_items <= D2D_RESTORE_MAX_ITEMS records (the argument list stays small, and a stream builds it once).
 * For every slot e < B with refill[e] != 0 every item is applied; nothing outside the named ranges is written, and the workgroups of
 * a slot whose refill byte is 0 return after reading that byte.  A slot has D2D_RESTORE_PARTS workgroups of one wave: a large item is cut into
 * that many runs of words, one per workgroup, and a small one belongs to one workgroup (item index modulo the parts), so the search
 * scratch of 150 KB a slot does not wait behind the small items.  The ranges are the caller's to keep inside their buffers: the
 * library cannot look into device memory before a launch. */
#define D2D_RESTORE_PARTS 8
int d2d_stream_restore(const d2d_restore_item *items, int32_t n_items, const uint8_t *refill, int32_t B, void *stream);

/* One wave per slot, every slot: cells[e] = the number of non-zero cells of slot e's dmap ([B] grids of W x H cells in the layout
 * `grid_tile`: 0 row-major, 16 tiled -- cells, not bytes: the padding of the tiled layout is not counted, whatever it holds).  The
 * count is d2d_stream_harvest's column D2D_STREAM_R_DMAP, the same text.  Reads st->dmap alone. */
int d2d_stream_explored(const d2d_state *st, int32_t B, int32_t W, int32_t H, int32_t grid_tile, int32_t *cells, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_WORLDS_TURN_H */
