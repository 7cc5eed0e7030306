/*
 * d2d_swept.h — the swept-trajectory map of the Primitive planner as an observation channel (VecDrone2DEnv(..., swept_obs=True)).
 *
 * Primitive.replan_check (traj_planner.py:220-233) builds, on every step, the map of the cells the stored trajectory will pass
 * through and when, and returns it; the env written for the gaze learner (envs/training_v3.py:141, :206-213) crops it around the
 * drone like the explored map and hands it to the policy as obs['swep_map'].  The plan stage of libd2d_hip.so replays the same walk
 * and keeps nothing; these two launches keep it:
 *
 *   d2d_swept_mark   between d2d_run_stages(PERCEIVE) and d2d_plan_stage[_live]: the map replan_check is about to return
 *   d2d_swept_crop   after d2d_run_stages(ACT): its L x L crop around the drone's cell, zero outside the map (L = d2d_cfg.L, the
 *                    window of obs_local)
 *
 * For an env with trajectory header (head, stored) and n = stored - head waypoints, waypoint i (from the head) is hit if an ACTIVE
 * tracker has fma(dy, dy, dx * dx) <= lim at time i * dt -- the operands, their order and `lim` (trk_lim where > 0, else the squared
 * threshold of drone_radius + trk_radius) are the plan stage's.  m = first hit + 1, or n.  The map is zero but for
 * map[cell(x_i), cell(y_i)] = ((int)(i * dt)) & 0xff for i = 0 .. m - 1 in order, the last write to a cell standing; a waypoint
 * outside the map writes nothing.  The wall test of replan_check never changes the map.
 *
 * d2d_swept_mark READS the plugin state: trk_radius, trk_prev, trk_lim and the trajectory are as before after it, so the plan stage
 * that follows does its bookkeeping and finds them as if the launch had not been there.  An env whose flags[D2D_F_DONE] is set
 * writes live = 0 and nothing else; d2d_swept_crop is a no-op for an env with live == 0.  A finished env therefore keeps the map,
 * crop and count of the step that ended its episode.
 *
 * Maps of up to 256 x 256 cells (the env's map is held in LDS whole); planner D2D_PLAN_PRIMITIVE.
 *
 * Additions to the library in the manner of include/d2d_stepped.h: no struct of d2d.h and no version changes with them, and a caller
 * looks them up as optional symbols.
 */
#ifndef D2D_SWEPT_H
#define D2D_SWEPT_H

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_SWEPT_MAX_SIDE 256

typedef struct {
  uint8_t *map;   /* [B][W][H] row-major, or whatever d2d_cfg.grid_tile says (the layout of d2d_state.dmap) */
  uint8_t *obs;   /* [B][L][L] */
  int32_t *count; /* [B] m of the last mark */
  uint8_t *live;  /* [B] 1: the last mark ran for this env */
} d2d_swept;

int d2d_swept_mark(const d2d_cfg *cfg, const d2d_state *st, const d2d_plan *plan, const d2d_swept *sw, void *stream);

int d2d_swept_crop(const d2d_cfg *cfg, const d2d_state *st, const d2d_swept *sw, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_SWEPT_H */
