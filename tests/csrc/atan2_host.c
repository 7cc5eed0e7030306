/* Host build of the device's atan2 restatement (csrc/d2d_atan2.h) for tests/test_atan2.py. */
#include <math.h>
#include <stdint.h>
#include "d2d_atan2.h"
void d2d_atan2_host_array(const double *y, const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = d2d_atan2(y[i], x[i]);
}
/* libm's atan2 behind CPython's special cases (Modules/mathmodule.c m_atan2): the expected values */
void d2d_atan2_libm_array(const double *y, const double *x, double *out, int64_t n) {
  const double pi = 3.141592653589793238462643383279502884197;
  for (int64_t i = 0; i < n; ++i) {
    const double yy = y[i], xx = x[i];
    double r;
    if (isnan(xx) || isnan(yy)) r = NAN;
    else if (isinf(yy)) r = isinf(xx) ? copysign(copysign(1., xx) == 1. ? 0.25 * pi : 0.75 * pi, yy) : copysign(0.5 * pi, yy);
    else if (isinf(xx) || yy == 0.) r = copysign(copysign(1., xx) == 1. ? 0. : pi, yy);
    else r = atan2(yy, xx);
    out[i] = r;
  }
}
