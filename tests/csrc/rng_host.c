/* Host build of the measurement noise's random stream (csrc/d2d_rng.h) for tests/test_rng_cpu.py. */
#include <stdint.h>
#include "d2d_rng.h"
/* m pairs from stream `st` (D2D_RNG_WORDS words) into out[m][2]; returns the pairs drawn */
int d2d_rng_host_draw(uint32_t *st, int m, double *out) { return d2d_rng_draw_seq(st, m, out); }
