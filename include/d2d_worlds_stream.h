/*
 * d2d_worlds_stream.h — the launches that turn a finished slot of a resident batch into the next seeded episode without
 * the host (libd2d_worlds.so; VecDrone2DEnv.stream_episodes, runner.EpisodeStream).
 *
 * A stream plays M episodes, episode k in the world of map_id0 + k, over B slots (B envs of one d2d_state).  slot_episode[e] says
 * which episode slot e plays, or -1 once the slot is retired (the queue ran dry).  Between two chunks of steps the caller queues
 *
 *   d2d_stream_harvest       every slot that is done and not retired writes the record of its episode to rows[slot_episode[e]]
 *   d2d_stream_assign        the same slots get the next episodes in slot order: slot_episode, map_id and a refill byte each
 *   d2d_worlds_build_masked  d2d_worlds_build for the slots whose refill byte is set, reading the map ids the assignment wrote
 *   d2d_stream_clear         zeroes the same slots' rows of a per-slot buffer that no masked reset covers
 *
 * and then puts back the state outside the world for the same slots (d2d_plan_reset, d2d_jerk_reset, d2d_gaze_reset with `refill`
 * as the mask).  All of them are asynchronous on the caller's stream and read nothing back; `counts` is the only thing the host
 * looks at.  An episode depends on nothing but its world, so neither the slot that plays it nor the time of its refill can change
 * its record.
 *
 * The done byte is byte D2D_STREAM_F_DONE of the state's own flags, [B][4] bytes (D2D_F_DONE of include/d2d.h, restated here).
 *
 * The record, D2D_STREAM_ROW_F int32 (columns D2D_STREAM_R_*): the counters C_STEPS, C_SM, C_BUF_N, C_BUF_TS of the slot, its
 * flags[0..2], and the number of non-zero cells of its dmap -- cells, not bytes: in the tiled layout (grid_tile = 16) the bytes of
 * the padding are not counted, whatever they hold.  These are the numbers a CSV row of the batch runners is made of.
 *
 * A slot whose world could not be built within d2d_world_spec.max_attempts (status D2D_WORLD_CAP) has its done byte set by
 * d2d_worlds_build_masked, so no launch steps it, and the next harvest records it as it is: every column 0.  Column
 * D2D_STREAM_R_STEPS == D2D_STREAM_BUILD_FAILED (0) is the marker: an episode that ran ends after at least one step.
 *
 * The functions are additions to the library: D2D_WORLDS_VERSION does not change with them, and a caller looks them up as optional
 * symbols.  Error codes and the thread-local message (d2d_worlds_last_error) are as in d2d_worlds.h.
 */
#ifndef D2D_WORLDS_STREAM_H
#define D2D_WORLDS_STREAM_H

#include <stdint.h>

#include "d2d_worlds.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_STREAM_F_DONE 3 /* D2D_F_DONE of include/d2d.h: byte of flags[e][4] that says slot e's episode has ended */

#define D2D_STREAM_ROW_F 8
#define D2D_STREAM_R_STEPS 0
#define D2D_STREAM_R_SM 1
#define D2D_STREAM_R_BUF_N 2
#define D2D_STREAM_R_BUF_TS 3
#define D2D_STREAM_R_FLAG0 4 /* flags[0], flags[1], flags[2] in columns 4, 5, 6 */
#define D2D_STREAM_R_DMAP 7
#define D2D_STREAM_BUILD_FAILED 0 /* value of column D2D_STREAM_R_STEPS of an episode whose world hit max_attempts */

#define D2D_STREAM_MAX_EPISODES 0x0fffffff /* M: rows is indexed with 32-bit episode numbers */

/* One wave per slot.  Reads st->flags, st->counters and st->dmap ([B] grids of W x H cells in the layout `grid_tile`: 0 row-major,
 * 16 tiled), and slot_episode [B].  A slot with its done byte set and 0 <= slot_episode[e] < M writes rows[slot_episode[e]]
 * ([M][D2D_STREAM_ROW_F] int32); any other slot reads its flags and its slot_episode and writes nothing. */
int d2d_stream_harvest(const d2d_state *st, const int32_t *slot_episode, int32_t B, int32_t W, int32_t H, int32_t grid_tile, int64_t M,
                       int32_t *rows, void *stream);

/* One workgroup.  counts = {cursor, finished} (device, int64): the next episode to hand out and the episodes harvested so far.
 * With h(e) = "done byte set and slot_episode[e] >= 0" (what d2d_stream_harvest just recorded), slot e with h(e) gets
 * episode k = cursor + |{e' < e : h(e')}|: for k < M slot_episode[e] = k, map_id[e] = map_id0 + k, refill[e] = 1; for k >= M the slot
 * is retired: slot_episode[e] = -1, refill[e] = 0, the done byte stays.  Every other slot: refill[e] = 0, nothing else written.
 * Then cursor = min(cursor + |h|, M) and finished += |h|.  No atomics: the result is a function of the inputs alone.
 * map_id0 + M <= 2^32 is the caller's to check. */
int d2d_stream_assign(const uint8_t *flags, int32_t B, int64_t M, uint32_t map_id0, int32_t *slot_episode, uint32_t *map_id,
                      uint8_t *refill, int64_t *counts, void *stream);

/* d2d_worlds_build for the slots e < spec->B with refill[e] != 0: the world fields of `st` and rows e of spec->tracker_radius,
 * spec->obstacles and spec->status, as d2d_worlds_build writes them, and the slot's four flag bytes where st->flags is not NULL:
 * all 0, or {0, 0, 0, 1} (done) for a slot whose status is D2D_WORLD_CAP.  Nothing of any other slot is written: its wave returns
 * after reading its refill byte. */
int d2d_worlds_build_masked(const d2d_world_spec *spec, const d2d_state *st, const uint8_t *refill, void *stream);

/* Zeroes rows e < B with refill[e] != 0 of a per-slot buffer `base`, [B][bytes_per_slot] (base aligned to 4 bytes, bytes_per_slot a
 * multiple of 4): the per-slot state that no masked reset covers -- the trajectory storage and search scratch of d2d_plan, the
 * scratch half of the RVO velocities -- so that a refilled slot holds what a fresh env holds there.  Nothing of any other slot is
 * written: its workgroup returns after reading its refill byte. */
int d2d_stream_clear(void *base, int64_t bytes_per_slot, const uint8_t *refill, int32_t B, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_WORLDS_STREAM_H */
