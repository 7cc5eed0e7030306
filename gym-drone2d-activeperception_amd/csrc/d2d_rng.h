/*
 * d2d_rng.h — restatement of the random stream behind the reference's measurement noise.
 *
 * Reference call site: utils.py:603-605, `sigma * np.random.randn(2)` for every agent the rays hit, in agent order, from the
 * global numpy stream the env seeded with map_id (envs/drone_v2.py:80).  Under a legacy seed that is numpy's legacy Gaussian
 * (numpy/random/src/legacy/legacy-distributions.c, legacy_gauss: Marsaglia's polar method) over MT19937
 * (numpy/random/src/mt19937/mt19937.c; Matsumoto & Nishimura's generator):
 *
 *   g()        the next tempered 32-bit output; the 624-word key is regenerated when the position reaches 624
 *   double     ((g() >> 5) * 67108864.0 + (g() >> 6)) / 9007199254740992.0
 *   attempt    x1 = 2 d - 1, x2 = 2 d - 1 (in that order), r2 = x1 x1 + x2 x2; rejected while r2 >= 1.0 || r2 == 0.0
 *   pair       f = sqrt(-2.0 * log(r2) / r2); randn(2) returns (f x2, f x1) -- the second from the generator's cache, so a call
 *              that starts with an empty cache ends with one
 *
 * log is the host libm's (d2d_log.h); sqrt and the divisions are IEEE.  Every attempt takes exactly four words whatever it
 * decides, so attempt j of a call reads words pos + 4 j .. pos + 4 j + 3; and 624 = 4 * 156, so from a position that is a
 * multiple of 4 -- the reference's world construction leaves 200 -- no attempt straddles a regeneration.  The device code in
 * d2d_hip.hip rests on both (64 attempts per wave pass, a ballot for the accepted ones); d2d_rng_draw_seq below is the plain
 * sequential form, for any position: the host build the tests compare numpy and the device with.
 *
 * One stream = D2D_RNG_WORDS uint32 (include/d2d.h): key[624], position, pairs drawn (wrapping), regenerations, zeros.
 *
 * Must be compiled with -ffp-contract=off (see d2d_log.h).
 */
#ifndef D2D_RNG_H
#define D2D_RNG_H

#include <math.h>
#include <stdint.h>

#ifndef D2D_RNG_QUAL
#define D2D_RNG_QUAL static inline
#endif
#ifndef D2D_LOG_QUAL
#define D2D_LOG_QUAL D2D_RNG_QUAL
#endif
#include "d2d_log.h"

#define D2D_RNG_KEY 624  /* words of the key */
#define D2D_RNG_POS 624  /* index of the position word */
#define D2D_RNG_NPAIR 625
#define D2D_RNG_NREGEN 626
#define D2D_RNG_M 397

/* genrand's tempering of key word y */
D2D_RNG_QUAL uint32_t d2d_rng_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

/* word i of the next key from key[i], key[i + 1] and key[i + 397] (indices mod 624; the last two may already be new words) */
D2D_RNG_QUAL uint32_t d2d_rng_twist(uint32_t ki, uint32_t ki1, uint32_t kim) {
  const uint32_t y = (ki & 0x80000000u) | (ki1 & 0x7fffffffu);
  return kim ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

/* random_double from two tempered outputs, in the order they were drawn */
D2D_RNG_QUAL double d2d_rng_double(uint32_t ga, uint32_t gb) {
  return ((double)(ga >> 5) * 67108864.0 + (double)(gb >> 6)) / 9007199254740992.0;
}

/* One attempt of the polar method from four tempered outputs.  Returns 1 and the pair randn(2) returns, or 0. */
D2D_RNG_QUAL int d2d_rng_attempt(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3, double *v0, double *v1) {
  const double x1 = 2.0 * d2d_rng_double(g0, g1) - 1.0;
  const double x2 = 2.0 * d2d_rng_double(g2, g3) - 1.0;
  const double r2 = x1 * x1 + x2 * x2;
  if (r2 >= 1.0 || r2 == 0.0) return 0;
  const double f = sqrt(-2.0 * d2d_log(r2) / r2);
  *v0 = f * x2;
  *v1 = f * x1;
  return 1;
}

/* Regenerations one call may run for `m` pairs before it gives up: a key that never yields an accepted attempt (all zero words:
 * not a state of the generator) must not be able to hang the caller.  156 attempts per regeneration, 3 in 4 accepted. */
D2D_RNG_QUAL int d2d_rng_regen_cap(int m) { return m / 64 + 8; }

#if !defined(__HIPCC__)
/* `m` pairs from stream `st` into out[m][2], sequentially, from any position <= 624.  Returns the pairs drawn (m, unless the
 * regeneration cap stopped the call; the rest of `out` is then 0). */
D2D_RNG_QUAL int d2d_rng_draw_seq(uint32_t *st, int m, double *out) {
  uint32_t pos = st[D2D_RNG_POS];
  int regen = 0, k = 0;
  for (int i = 0; i < 2 * m; ++i) out[i] = 0.0;
  while (k < m) {
    uint32_t g[4];
    for (int j = 0; j < 4; ++j) {
      if (pos >= D2D_RNG_KEY) {
        if (regen >= d2d_rng_regen_cap(m)) goto out;
        for (int i = 0; i < D2D_RNG_KEY; ++i)
          st[i] = d2d_rng_twist(st[i], st[(i + 1) % D2D_RNG_KEY], st[(i + D2D_RNG_M) % D2D_RNG_KEY]);
        pos = 0;
        regen += 1;
      }
      g[j] = d2d_rng_temper(st[pos++]);
    }
    if (d2d_rng_attempt(g[0], g[1], g[2], g[3], out + 2 * k, out + 2 * k + 1)) k += 1;
  }
out:
  st[D2D_RNG_POS] = pos;
  st[D2D_RNG_NPAIR] += (uint32_t)k;
  st[D2D_RNG_NREGEN] += (uint32_t)regen;
  return k;
}
#endif

#endif /* D2D_RNG_H */
