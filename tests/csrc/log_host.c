/* Host build of the device's log restatement (csrc/d2d_log.h) for tests/test_log.py. */
#include <math.h>
#include <stdint.h>
#include "d2d_log.h"
void d2d_log_host_array(const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = d2d_log(x[i]);
}
/* libm's log: the expected values */
void d2d_log_libm_array(const double *x, double *out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = log(x[i]);
}
