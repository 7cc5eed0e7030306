/*
 * d2d_seen.h — C ABI of the time-since-observed map as an observation channel (libd2d_seen.so): for every env of a batch, what
 * yaw_planner.Oxford keeps as `last_time_observed_map` ("how long ago did I last look at this cell", yaw_planner.py:49, :92-97),
 * kept for a learner whatever policy chooses the action, and its crop around the drone.
 *
 * Definition.  For an env that has taken k steps the age map is what Oxford.last_time_observed_map holds right after the "update
 * t_i" part of its (k + 1)-th plan() call: the call the reference makes from the pose the env is in now.  Kept as integers:
 *
 *   seen[B][W][H]   the number of the call that last saw the cell, 0 = never; the call number is counters[D2D_C_STEPS] + 1
 *   value after call c of a cell   tab[0][c - seen] where it was seen (0 where seen == c), tab[1][c] where it never was
 *   tab[2][tab_len]                the host's table of the reference's own additions: 0 + dt + dt ..., 5 + dt + dt ...
 *
 * d2d_seen_update, one wave per env, for env e with call = steps + 1:
 *   skip     call <= last_call[e] or call >= tab_len (or call < 1): nothing of the env is written.  Idempotent; covers finished envs,
 *            whose counter stands still in every launch that leaves them alone, and envs stepped past the table
 *   mark     every cell of the box around the drone that can be in view takes Oxford.get_view_map's decision (yaw_planner.py:67-79)
 *            with the operands in the reference's order: the cell's origin (i * scale, j * scale), the direction
 *            cos(radians(yaw)), -sin(radians(yaw)), d2 <= 0 is seen, d2 <= depth ** 2, arccos(dot / sqrt(d2)) <= half_fov through the
 *            host's 64-double decision window (a quotient above 1 is NaN: not seen).  Marked cells get seen = call
 *   refreshed[e]   the cells marked now whose previous value was 0 or < call - 1: the coverage this pose bought.  A sum of
 *            population counts, so it does not depend on any order
 *   obs[e]   [L][L] float32, L = d2d_cfg.L: the window around the drone's cell (int(x // scale), int(y // scale)), 0 outside the map
 *            (np.pad(..., constant_values=0) as get_local_map and envs/training_v3.py:206-209 have it), each value np.float32 of the
 *            float64 table value.  A cell this launch marks is decided by the view test again, not read back
 *   last_call[e] = call
 *
 * `seen` is row-major [W][H] whatever d2d_cfg.grid_tile says, and nothing is held in LDS whole: there is no map-size limit beyond
 * 32-bit cell indices.  A value of `seen` that is not a call number of this env's past (negative, or above the call) is read as
 * "never seen" (negative or zero) or as "seen now" (above the call): every table index stays inside the table.
 *
 * The launch reads d2d_state.drone and d2d_state.counters alone.  Conventions as in d2d_gaze.h: plain C, the caller owns all memory,
 * DEVICE pointers, asynchronous on the caller's stream, 0 or a negative error (-1 NULL pointer or bad argument, -2 another
 * D2D_ABI_VERSION in the cfg, -3 HIP launch error, -4 a size the launch cannot hold) with a thread-local message and no launch.  The
 * library is separate from libd2d_hip.so and reports its own version.
 */
#ifndef D2D_SEEN_H
#define D2D_SEEN_H

#include <stdint.h>

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_SEEN_VERSION 1

typedef struct d2d_seen {
  /* ---- the channel's per-env state and outputs ---- */
  int32_t *seen;       /* [B][W][H] */
  int32_t *last_call;  /* [B] the call of the latest update, 0 = none */
  int32_t *refreshed;  /* [B] */
  float *obs;          /* [B][L][L] */
  /* ---- the host's tables ---- */
  const double *tab;   /* [2][tab_len] */
  int64_t acos_key_lo; /* np.arccos(q) <= half_fov for the 64 doubles from the one with this ordered key: bit k of acos_mask; */
  uint64_t acos_mask;  /* every q <= 1 above the window is inside the cone, every q below it outside */
  int32_t tab_len;
  int32_t reserved;    /* 0 */
} d2d_seen;

int d2d_seen_version(void);
const char *d2d_seen_last_error(void);

/* B >= 0 (0: nothing to do), tab_len >= 2.  -4: W * H or L * L beyond 32-bit indices */
int d2d_seen_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_seen *seen, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_SEEN_H */
