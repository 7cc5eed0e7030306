/*
 * d2d_scan.h — C ABI of the per-ray scan of the limited-FOV raycast (libd2d_scan.so): for every env of a batch, what the reference
 * keeps as `env.drone.rays` after a step (utils.py:593-594, :620-713, :746) -- where each ray ended, on what, and which agents it
 * found -- and a two-row observation (range and outcome per ray) for a learner.
 *
 * Definition.  scan(e) after a step is Raycast.castRays of that step.  Its inputs are the pose the drone had BEFORE the step's
 * step_pos / step_yaw (`pose`, a snapshot the caller takes in front of the step), the agents AFTER the step's move
 * (d2d_state.agents as the step left them) and the static cells of map_gt: OCCUPIED cells never change (utils.py:527-540 never
 * overwrites a 1) and the stop test `wall == 1` reads only them, so the scan is recomputed exactly behind the step.
 *
 * d2d_scan_update, one wave per env, lane = ray, ceil(R / 64) passes; for env e:
 *   skip     counters[D2D_C_STEPS] == last_step[e], or below 1: the env is left alone entirely -- the wave returns before it reads
 *            anything else.  Idempotent; covers finished envs, whose counter stands still in every launch that leaves them alone,
 *            and a fresh world, which has no rays yet (the reference's `self.rays = {}`)
 *   ray i    utils.py:620-713 with the operands in the reference's order: player_angle = 2 pi - yaw * (pi / 180),
 *            ang = positive_angle(player_angle + (ray_off0 + ray_dth * i)), slope = tan(ang) (the host libm's bits), the
 *            |slope| > 1 branch with 1.0 / slope, steps of scale - 1, samples x = x + x_step while 0 < x < W_px && 0 < y < H_px on
 *            doubles, the cell int(x // scale), the circle test dx * dx + dy * dy <= r2 with r2 from the agents' plane
 *   end[e][i]    (x_hit, y_hit): the reference's iterated sums, bit for bit; (-1, -1) for a ray that leaves the map without
 *            stopping or whose drone is not strictly inside the map
 *   kind[e][i]   0 no stop; 1 stopped on an OCCUPIED cell; 2 stopped inside at least one agent (the agent test comes first at every
 *            sample, :658-664, sample 0 -- the drone's own position -- included); 3 range stop, dist >= depth ** 2 on a cell that
 *            is not OCCUPIED
 *   hit[e][i]    hit_words = max(1, ceil(N / 32)) words: bit k % 32 of word k / 32 is set iff agent k's circle holds the stopping
 *            sample -- every such agent, not only the first.  All words are rewritten by every update, by the ray's own lane: no
 *            atomics
 *   obs[e][0][i] float32 of sqrt((x_hit - x0) ** 2 + (y_hit - y0) ** 2) evaluated in binary64; for kind 0 from the last sample taken
 *            inside the map, 0 when none was taken
 *   obs[e][1][i] float32 of kind
 *   last_step[e] = counters[D2D_C_STEPS]
 *
 * The two obs rows are this port's own derivation; everything else is the reference's.  ONE DEVIATION: at a range stop the
 * reference's 'wall' is the raw map_gt value of that moment, 2 or -- where the cell still carries the previous step's dynamic mark
 * -- 3.  That layer is overwritten later in the same step and cannot be recovered behind it, so `wall` is reported from `kind` as
 * {0: 0, 1: 1, 2: 0, 3: 2}: right except on those cells (13 of 487 range stops of the recorded teleport episode).  Nothing in the
 * reference reads the field.
 *
 * The launch reads d2d_state.agents (the x, y and r ** 2 planes), d2d_state.gt in the cfg's layout (grid_tile 0 or 16, partial
 * edge tiles included) and d2d_state.counters.  It writes nothing of the state and never touches dmap.  A sample's cell index is
 * formed only by a live lane whose sample lies inside the map, and is clamped to the grid.
 *
 * Conventions as in d2d_seen.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 NULL pointer or bad argument, -2 another D2D_ABI_VERSION in the cfg, -3 HIP launch error, -4 a size that 32-bit
 * indexing cannot hold) with a thread-local message and no launch.  The library is separate from libd2d_hip.so and reports its own
 * version.
 */
#ifndef D2D_SCAN_H
#define D2D_SCAN_H

#include <stdint.h>

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_SCAN_VERSION 1

typedef struct d2d_scan {
  const double *pose;   /* [B][8], layout of d2d_state.drone: x, y, yaw are read */
  double *end;          /* [B][R][2] */
  uint8_t *kind;        /* [B][R] */
  uint32_t *hit;        /* [B][R][hit_words] */
  float *obs;           /* [B][2][R] */
  int32_t *last_step;   /* [B] counters[D2D_C_STEPS] of the latest update, 0 = none */
  int32_t hit_words;    /* max(1, ceil(N / 32)) */
  int32_t reserved;     /* 0 */
} d2d_scan;

int d2d_scan_version(void);
const char *d2d_scan_last_error(void);

/* B >= 0 (0: nothing to do), R >= 1, scale > 1.  -4: W * H, R * hit_words or N beyond 32-bit indices */
int d2d_scan_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_scan *scan, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_SCAN_H */
