/* Host build of the device's pow(x, 2.0) restatement (csrc/d2d_pow2.h) for tests/test_pow2.py. */
#include <math.h>
#include <stdint.h>
#include "d2d_pow2.h"
void d2d_pow2_host_array(const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = d2d_pow2(x[i]);
}
/* libm's pow(x, 2.0): the expected values (the exponent is volatile so that the compiler cannot turn the call into x * x) */
void d2d_pow2_libm_array(const double *x, double *out, int64_t n) {
  volatile double two = 2.0;
  for (int64_t i = 0; i < n; ++i) out[i] = pow(x[i], two);
}
