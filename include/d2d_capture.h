/*
 * d2d_capture.h — the terminal frames of streamed episodes, chosen and drawn on the device (libd2d_render.so; drone2d_amd/capture.py,
 * VecDrone2DEnv.stream_episodes(capture=), action_stream(capture=), runner.EpisodeStream with params.record_img).
 *
 * A stream rebuilds a finished slot in place at its next turn; until then the slot is frozen, and the renderer draws any slot without
 * writing to it.  In front of every d2d_stream_harvest the caller queues three launches that read nothing back:
 *
 *   d2d_capture_select     which of the slots that the harvest is about to record are drawn, and where in the gallery
 *   d2d_render_list_sel    d2d_render_list over the chosen slots; an entry that names no slot (-1) is skipped
 *   d2d_render_frame_sel   d2d_render_frame over the same entries, each painted into the gallery frame the selection gave it
 *
 * The reference saves a screenshot when the drone collides (params.record_img, envs/training_v3.py:180-187).  It saves self.screen,
 * which holds the picture of the previous render() call; this draws the terminal state itself.
 *
 * The functions are additions to the library: D2D_RENDER_VERSION does not change with them, and a caller looks them up as optional
 * symbols.  Error codes and the thread-local message (d2d_render_last_error) are as in d2d_render.h.
 */
#ifndef D2D_CAPTURE_H
#define D2D_CAPTURE_H

#include <stdint.h>

#include "d2d_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_RENDER_SKIPPED 3 /* status of an entry of d2d_render_list_sel whose slot number is -1: nothing of it was read or drawn */

/* how an episode ended: the first of these that holds, read from the bytes a CSV row is made of */
#define D2D_CAPTURE_STATIC 1    /* flags[D2D_F_COLLISION] == 1 */
#define D2D_CAPTURE_DYNAMIC 2   /* flags[D2D_F_COLLISION] == 2 */
#define D2D_CAPTURE_DEAD_LOCK 3 /* flags[D2D_F_DEADLOCK] != 0 */
#define D2D_CAPTURE_FREEZING 4  /* flags[D2D_F_FREEZING] != 0 */
#define D2D_CAPTURE_GOAL 5      /* counters[D2D_C_SM] == D2D_SM_GOAL_REACHED */
#define D2D_CAPTURE_OTHER 6     /* none of the above (the flight time ran out; under RVO a failed RVO_update) */
#define D2D_CAPTURE_KINDS 6

#define D2D_CAPTURE_META_F 4 /* meta row: episode, kind, steps, slot */
#define D2D_CAPTURE_M_EPISODE 0
#define D2D_CAPTURE_M_KIND 1
#define D2D_CAPTURE_M_STEPS 2
#define D2D_CAPTURE_M_SLOT 3

#define D2D_CAPTURE_COUNTS 3 /* counts: taken, dropped, matched */

/* One workgroup of one wave: 64 slots a pass, in slot order, ranks from ballots and prefix pop-counts, no atomics -- the result is a
 * function of the inputs alone.  Reads cfg->B, st->flags, st->counters, st->drone and slot_episode ([B], or NULL: slot e plays
 * "episode e", for a batch that is not a stream); writes nothing of st.
 *
 * Slot e MATCHES when its done byte is set, slot_episode[e] >= 0 (or slot_episode is NULL), counters[D2D_C_STEPS] > 0 (a world that
 * hit the attempt cap never ran) and bit (kind - 1) of `kinds` is set for its kind (D2D_CAPTURE_*).  With r the rank of a matching
 * slot among this call's matches in slot order and taken = counts[0] as the call found it, the slot is ACCEPTED when r < S and
 * taken + r < capacity: sel_slot[r] = e, sel_dst[r] = taken + r, meta[taken + r] = {episode, kind, steps, slot} and
 * pose[taken + r] = {x, y, yaw}, the state's float64 bits.  Every entry of sel_slot and sel_dst ([S]) at or beyond the number
 * accepted becomes -1.  Then counts ([D2D_CAPTURE_COUNTS] int64, device) move on: taken += accepted, dropped += matches - accepted,
 * matched += matches.  meta is [capacity][D2D_CAPTURE_META_F] int32, pose [capacity][3] float64; rows not named are left alone.
 * A negative counts[0] accepts nothing. */
int d2d_capture_select(const d2d_cfg *cfg, const d2d_state *st, const int32_t *slot_episode, uint32_t kinds, int32_t S, int64_t capacity,
                       int32_t *sel_slot, int32_t *sel_dst, int32_t *meta, double *pose, int64_t *counts, void *stream);

/* d2d_render_list, except that an entry with call->slots[i] == -1 is skipped: its wave returns after reading the slot number,
 * count[i] = 0, status[i] = D2D_RENDER_SKIPPED, nothing else of it is written.  Any other slot number outside the batch stays
 * D2D_RENDER_BAD_SLOT. */
int d2d_render_list_sel(const d2d_cfg *cfg, const d2d_state *st, const d2d_render_call *call, void *stream);

/* d2d_render_frame, except that entry i paints frame dst[i] of call->frame ([capacity][Hf][Wf][3]) instead of frame i, and every
 * workgroup of an entry with call->slots[i] == -1, or with dst[i] outside [0, capacity), returns before it reads a list or stores a
 * pixel.  dst is [S] int32 on the device. */
int d2d_render_frame_sel(const d2d_cfg *cfg, const d2d_state *st, const d2d_render_call *call, const int32_t *dst, int64_t capacity,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_CAPTURE_H */
