/*
 * d2d_stepped.h — the plugin stages of libd2d_hip.so for an episode loop that is driven step by step from the host
 * (VecDrone2DEnv.run_episodes with the Primitive plugins: gaze -> [RVO] -> perceive -> plan -> act, one launch each).
 *
 *   d2d_gaze_stage_live   d2d_gaze_stage for the envs that are not done
 *   d2d_plan_stage_live   d2d_plan_stage for the envs that are not done
 *
 * Arguments, checks and error codes are those of d2d_gaze_stage / d2d_plan_stage (include/d2d.h).  An env whose
 * flags[D2D_F_DONE] is set keeps everything the stage would otherwise write: its action, its plugin state (trajectory, header,
 * boxes, seen_step, the Owl scores and held decision, the tracker bookkeeping) and plan_ok / wp_valid / wp.  This is the mode
 * d2d_closed_loop(D2D_DONE_FREEZE) runs its per-stage path in; together with d2d_run_stages(... | D2D_ST_SKIP_DONE) a finished env
 * stays as its episode left it however many steps the rest of the batch still plays.
 *
 * The two are additions to the library, outside the surface the CPU oracle mirrors (include/d2d.h) and outside the test hooks
 * (include/d2d_hooks.h): no struct and no version changes with them, and a caller looks them up as optional symbols.
 */
#ifndef D2D_STEPPED_H
#define D2D_STEPPED_H

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

int d2d_gaze_stage_live(const d2d_cfg *cfg, const d2d_state *st, const d2d_plan *plan, void *stream);

int d2d_plan_stage_live(const d2d_cfg *cfg, const d2d_state *st, const d2d_plan *plan, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_STEPPED_H */
