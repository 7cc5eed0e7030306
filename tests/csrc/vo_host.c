/* Host build of the velocity-obstacle metric's arithmetic (csrc/metrics/d2d_vo.h) for tests/test_vo_host_build.py: the three
 * entry points of include/d2d_metrics.h as loops over host arrays. */
#include <math.h>
#include <stdint.h>
#include "d2d_vo.h"
void vo_host_geometry(const double *agents, const double *pos, double rA, int32_t B, int32_t N, int32_t P, double *arg,
                      double *theta_ba, uint8_t *collided) {
  d2d_vo_geometry_seq(agents, pos, rA, B, N, P, arg, theta_ba, collided);
}
void vo_host_cones(const double *theta_ba, const double *half, const uint8_t *collided, int32_t B, int32_t N, int32_t P, double *cone) {
  d2d_vo_cones_seq(theta_ba, half, collided, B, N, P, cone);
}
void vo_host_count(const double *agents, const double *cand, const double *cone, const uint8_t *collided, int32_t B, int32_t N,
                   int32_t P, int32_t C, int32_t *count) {
  d2d_vo_count_seq(agents, cand, cone, collided, B, N, P, C, count);
}
int vo_host_version(void) { return D2D_METRICS_VERSION; }
