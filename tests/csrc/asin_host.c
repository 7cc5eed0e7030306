/* Host build of the device's asin restatement (csrc/metrics/d2d_asin.h) for tests/test_asin.py. */
#include <math.h>
#include <stdint.h>
#include "d2d_asin.h"
void d2d_asin_host_array(const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = d2d_asin(x[i]);
}
/* libm's asin: the expected values (math.asin raises where this returns NaN for |x| > 1) */
void d2d_asin_libm_array(const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = asin(x[i]);
}
