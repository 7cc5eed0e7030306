/*
 * d2d_jerk_live.h — the plan launch of include/d2d_jerk.h for a batch in which some envs have finished their episode
 * (libd2d_jerk.so; VecDrone2DEnv.run_episodes with planner='Jerk_Primitive').
 *
 *   d2d_jerk_plan_live   d2d_jerk_plan for the envs that are not done; nothing of a finished env is read or written
 *
 * `flags` is the state's own d2d_state.flags, [B][4] bytes; byte D2D_JERK_LIVE_F_DONE of an env decides (D2D_F_DONE of include/d2d.h,
 * restated here so that this header stands alone).
 *
 * A live env gets bit for bit what d2d_jerk_plan gives it: plan_ok, wp_valid, wp, choice, stat and the trk_radius / trk_prev
 * bookkeeping.  The launch has one wave per env and the wave is the whole workgroup, so the test is uniform: a finished env's wave
 * loads its done byte and returns -- before the tracker loop, before it writes LDS and before the first barrier.  Of a finished env
 * nothing but that byte is read, and none of the seven buffers is written: its last plan, its last choice and its trackers' radii
 * stay those of the step that ended its episode.
 *
 * flags == NULL is refused with -1 (d2d_jerk_plan is the launch without a mask).  Every other refusal, the error codes and the
 * thread-local message (d2d_jerk_last_error) are d2d_jerk_plan's.  The function is an addition to the library: D2D_JERK_VERSION does
 * not change with it, and a caller looks it up as an optional symbol.
 */
#ifndef D2D_JERK_LIVE_H
#define D2D_JERK_LIVE_H

#include <stdint.h>

#include "d2d_jerk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_JERK_LIVE_F_DONE 3 /* D2D_F_DONE of include/d2d.h: byte of flags[b][4] that says env b's episode has ended */

/* d2d_jerk_plan with flags [B][4] (u8): the entries of the envs whose done byte is 0 are written, no entry of any other env. */
int d2d_jerk_plan_live(const d2d_jerk_call *call, const uint8_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_JERK_LIVE_H */
