/* Host build of the redraw's scalar statement (csrc/worlds/d2d_worlds.h d2d_w_redraw) for tests/test_validation_redraw_cpu.py. */
#include <stddef.h>
#include <stdint.h>
#include "worlds/d2d_worlds.h"

/* agent k of n: the four tempered words g[4 k ..] -> out[2 k] = pvx, out[2 k + 1] = pvy */
void d2d_redraw_host_words(int n, const uint32_t *g, double *out) {
  for (int k = 0; k < n; ++k) d2d_w_redraw(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3], &out[2 * k], &out[2 * k + 1]);
}

/* the statement's angle (r * 2.0) * pi of every r, and the library's cos and sin of it */
void d2d_redraw_host_angles(int n, const double *r, double *angle, double *c, double *s) {
  for (int k = 0; k < n; ++k) {
    angle[k] = (r[k] * 2.0) * 3.141592653589793;
    c[k] = d2d_cos(angle[k]);
    s[k] = d2d_sin(angle[k]);
  }
}
