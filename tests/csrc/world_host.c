/* Host build of the world construction's sequential form (csrc/worlds/d2d_worlds.h) for tests/test_world_seq_cpu.py. */
#include <stdint.h>
#include <stdlib.h>
#include "worlds/d2d_worlds.h"

/* every env of `spec` into the HOST arrays behind `st`; returns 0, or -1 without memory */
int d2d_worlds_host_build(const d2d_world_spec *spec, const d2d_state *st) {
  uint32_t *buf = (uint32_t *)malloc(sizeof(uint32_t) * D2D_W_BUF);
  double *acc = (double *)malloc(sizeof(double) * D2D_W_ACC_F * (size_t)(spec->n_rand + 1));
  if (!buf || !acc) return -1;
  for (int e = 0; e < spec->B; ++e) d2d_worlds_build_seq_env(spec, st, e, buf, acc);
  free(buf);
  free(acc);
  return 0;
}

/* the Python stream alone, no libm: key[624] as random.seed(seed) leaves it, then nd random() and nr _randbelow(n) */
void d2d_worlds_host_python(uint32_t seed, uint32_t *key_out, int nd, double *d, int nr, uint32_t n, uint32_t *r) {
  uint32_t key[D2D_RNG_KEY];
  int pos = D2D_RNG_KEY;
  d2d_w_seed_python(key, seed);
  for (int i = 0; i < D2D_RNG_KEY; ++i) key_out[i] = key[i];
  const int k = d2d_w_bit_length(n);
  for (int q = 0; q < 2 * nd + nr;) {
    if (pos >= D2D_RNG_KEY) {
      for (int i = 0; i < D2D_RNG_KEY; ++i)
        key[i] = d2d_rng_twist(key[i], key[(i + 1) % D2D_RNG_KEY], key[(i + D2D_RNG_M) % D2D_RNG_KEY]);
      pos = 0;
    }
    const uint32_t g = d2d_rng_temper(key[pos++]);
    if (q < 2 * nd) {
      if (q & 1) d[q / 2] = d2d_rng_double(r[0], g);
      else r[0] = g;
      q += 1;
    } else if ((g >> (32 - k)) < n) {
      r[q - 2 * nd] = g >> (32 - k);
      q += 1;
    }
  }
}

/* the numpy stream as the construction leaves it: key after its first regeneration, position 200 */
void d2d_worlds_host_numpy(uint32_t seed, uint32_t *st) {
  uint32_t key[D2D_RNG_KEY];
  d2d_w_init_genrand(key, seed);
  for (int i = 0; i < D2D_RNG_KEY; ++i)
    key[i] = d2d_rng_twist(key[i], key[(i + 1) % D2D_RNG_KEY], key[(i + D2D_RNG_M) % D2D_RNG_KEY]);
  for (int i = 0; i < D2D_RNG_WORDS; ++i) st[i] = i < D2D_RNG_KEY ? key[i] : i == D2D_RNG_POS ? D2D_W_NP_POS : 0u;
}
