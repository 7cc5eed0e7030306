/* Host build of the traversability / survival-fit arithmetic (csrc/metrics/d2d_difficulty.h) for tests/test_difficulty_host_build.py:
 * the two entry points of include/d2d_metrics.h as loops over host arrays. */
#include <math.h>
#include <stdint.h>
#include "d2d_difficulty.h"
void difficulty_host_trav_steps(const uint8_t *gt, int32_t B, int32_t W, int32_t H, const int32_t *starts, int32_t S, int32_t *steps) {
  d2d_trav_steps_seq(gt, B, W, H, starts, S, steps);
}
/* work: 5 * N doubles */
void difficulty_host_fit_first_hit(const double *agents, const double *pos, double drone_radius, double W_px, double H_px, double scale,
                                   double dt, int32_t B, int32_t N, int32_t P, int32_t checks, int32_t *first, double *agents_out,
                                   double *work) {
  d2d_fit_first_hit_seq(agents, pos, drone_radius, W_px, H_px, scale, dt, B, N, P, checks, first, agents_out, work);
}
int difficulty_host_version(void) { return D2D_METRICS_VERSION; }
