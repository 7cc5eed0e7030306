/* Host build of the RVO motion profile's arithmetic (csrc/rvo/d2d_rvo.h) for tests/test_rvo_host_build.py: the two entry points of
 * include/d2d_rvo.h as loops over host arrays. */
#include <math.h>
#include <stdint.h>
#include "d2d_rvo.h"
/* work: 6 * (N - 1 + P) doubles */
int rvo_host_velocity(const double *agents, const double *vel, const int32_t *pillars, int32_t B, int32_t N, int32_t P, double *vel_out,
                      double *work) {
  return d2d_rvo_velocity_seq(agents, vel, pillars, B, N, P, vel_out, work);
}
void rvo_host_agents_step(double *agents, const double *vel, double W_px, double H_px, double scale, double dt, int32_t B, int32_t N) {
  d2d_rvo_agents_step_seq(agents, vel, W_px, H_px, scale, dt, B, N);
}
int rvo_host_radii(double norm_v, double *delta) { return d2d_rvo_radii(norm_v, delta); }
int rvo_host_version(void) { return D2D_RVO_VERSION; }
int rvo_host_max_cones(void) { return D2D_RVO_MAX_CONES; }
