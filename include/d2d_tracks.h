/*
 * d2d_tracks.h — C ABI of the tracker-forecast map as an observation channel (libd2d_tracks.so): for every env of a batch, where and
 * how soon the Kalman trackers' forecasts come within the planner's keep-out distance of a cell -- what Planner.is_free
 * (traj_planner.py:54-58) and Primitive.replan_check (:225-229) test every candidate and every stored waypoint against -- cut around
 * the drone as a learner's other maps are.
 *
 * Definition.  For an env in the state the last step left it, with
 *   thr_q     = drone_radius + trackers[q].radius + margin           (two additions, left to right)
 *   pos(i, j) = OccupancyGridMap.get_real_pos(i, j) = (scale * (i + 0.5), scale * (j + 0.5))       (utils.py:542)
 *
 *   F[i, j] = 1 + min { k in 0 .. samples - 1 : some ACTIVE tracker q has norm(pos(i, j) - trackers[q].estimate_pos(k * dt)) <= thr_q }
 *   F[i, j] = 0 where there is no such k
 *
 * estimate_pos(t) is utils.py:220-223, mu[:2] + t * mu[2:] of the tracker's latest mu (the first four doubles of its d2d_state.kf
 * record), a multiplication and an addition; t = k * dt is the product replan_check forms (i * self.params.dt), so sample k is the
 * instant of waypoint k of the swept-trajectory map (d2d_swept.h).  margin = 5 + var_cam is the keep-out of Planner.is_free,
 * margin = 0 the test of replan_check.  trackers[q].radius is the device planners' trk_radius[B][N] (d2d_plan.trk_radius,
 * d2d_jerk_call.trk_radius): exact for every active tracker once a step has run.  The distance test is the plan stage's:
 * fma(dy, dy, dx * dx) <= (the largest s with sqrt(s) <= thr_q).
 *
 * win[e] is the L x L window of F (L = d2d_cfg.L) anchored at (int(x // scale) - edge, int(y // scale) - edge), edge = (L - 1) / 2,
 * 0 outside the map: np.pad(..., constant_values=0) and the cut of get_local_map and envs/training_v3.py:206-209.  Only the window
 * is computed: there is no [B][W][H] plane and no map-size limit.  cells[e] counts the window's nonzero cells.
 *
 * d2d_tracks_update, one wave per env.  Env e is updated iff force != 0 or counters[e][D2D_C_STEPS] != last_step[e]; otherwise
 * nothing of it is written.  An updated env gets its whole window, cells[e] and last_step[e] = its step counter.  So a finished env,
 * whose counter stands still, keeps its terminal window (and the terminal step itself is still computed); a refilled or reset slot,
 * whose counter jumped back and which has no active tracker (utils.py:182), comes out all zero; a repeated launch changes nothing.
 *
 * The launch reads d2d_state.drone, counters, active and kf, and trk_radius; nothing else.  N == 0 gives zeros; kf == NULL (or
 * active == NULL) with N > 0 is -1.  Conventions as in d2d_seen.h: plain C, the caller owns all memory, DEVICE pointers,
 * asynchronous on the caller's stream, 0 or a negative error (-1 NULL pointer or bad argument, -2 another D2D_ABI_VERSION in the
 * cfg, -3 HIP launch error, -4 a size the launch cannot hold) with a thread-local message and no launch.  The library is separate
 * from libd2d_hip.so and reports its own version.
 */
#ifndef D2D_TRACKS_H
#define D2D_TRACKS_H

#include <stdint.h>

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_TRACKS_VERSION 1
#define D2D_TRACKS_MAX_SAMPLES 255

typedef struct d2d_tracks {
  const double *trk_radius; /* [B][N] */
  uint8_t *win;             /* [B][L][L] the window of F */
  int32_t *cells;           /* [B] nonzero cells of the window */
  int32_t *last_step;       /* [B] counters[D2D_C_STEPS] at the latest update, -1 = none */
  double margin;
  int32_t samples;          /* 1 .. 255 */
  int32_t force;            /* != 0: update every env */
} d2d_tracks;

int d2d_tracks_version(void);
const char *d2d_tracks_last_error(void);

/* B >= 0 (0: nothing to do).  -4: L * L beyond 32-bit indices, or more agents than one wave's tracker staging holds in LDS */
int d2d_tracks_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_tracks *tracks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_TRACKS_H */
