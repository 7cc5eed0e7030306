/* Host build of the velocity-obstacle cones with the device's asin (csrc/metrics/d2d_vo.h + d2d_asin.h) for
 * tests/test_vo_device_asin_host_build.py: vo_host.c's loops, plus d2d_vo_cones_arg and d2d_asin_array as loops over host arrays. */
#include "vo_host.c"
void vo_host_cones_arg(const double *theta_ba, const double *arg, const uint8_t *collided, int32_t B, int32_t N, int32_t P,
                       double *half_out, double *cone) {
  d2d_vo_cones_arg_seq(theta_ba, arg, collided, B, N, P, half_out, cone);
}
void vo_host_asin(const double *x, int64_t n, double *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = d2d_asin(x[i]);
}
