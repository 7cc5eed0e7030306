/* Host build of the Jerk_Primitive planner's arithmetic (csrc/jerk/d2d_jerk.h) for tests/test_jerk_host_build.py: the two entry
 * points of include/d2d_jerk.h as loops over host arrays, and the scalar pieces the tests look at on their own. */
#include <math.h>
#include <stdint.h>
#include "d2d_jerk.h"
/* work: 5 * max(N, 1) doubles */
int jerk_host_plan(const d2d_jerk_call *call, double *work) { return d2d_jerk_plan_seq(call, work); }
void jerk_host_reset(double *trk_radius, uint8_t *trk_prev, const double *trk_radius0, const uint8_t *mask, int32_t mask_stride, int32_t B,
                     int32_t N) {
  d2d_jerk_reset_seq(trk_radius, trk_prev, trk_radius0, mask, mask_stride, B, N);
}
double jerk_host_mod360(double a) { return d2d_jerk_mod360(a); }
double jerk_host_phi(double px, double py, double gx, double gy) { return d2d_jerk_phi(px, py, gx, gy); }
double jerk_host_cost(int32_t i, double pm) { return d2d_jerk_cost(i, pm); }
int jerk_host_pattern(double pm) { return d2d_jerk_pattern(pm); }
int jerk_host_version(void) { return D2D_JERK_VERSION; }
int jerk_host_call_bytes(void) { return (int)sizeof(d2d_jerk_call); }
