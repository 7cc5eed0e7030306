/*
 * d2d_pow2.h — restatement of the libm pow(x, 2.0) that the reference's Owl gaze policy calls.
 *
 * Reference call site: yaw_planner.py:209 `norm(drone.velocity / 10) ** 2`.  numpy's scalar power of a float64 calls the host
 * libm's pow, and pow(x, 2.0) is NOT x * x: glibc's pow is accurate to about 0.52 ulp, not correctly rounded, so roughly one
 * argument in 1100 gets the neighbour of the rounded square.  The cost that holds this factor is compared with `==`, so the
 * device has to return libm's bits.
 *
 * glibc 2.35's double pow (sysdeps/ieee754/dbl-64/e_pow.c, from the ARM optimized routines, MIT / LGPL-2.1-or-later) computes
 * exp(y log x): log_inline gives log x as hi + lo from a 128-row table (__pow_log_data) and a degree-7 polynomial, exp_inline
 * exponentiates y hi + y lo with a second 128-row table (__exp_data) and a degree-5 polynomial.  x86-64 libm dispatches pow
 * through an ifunc; on every CPU with FMA + AVX2 it resolves to the variant built with -mfma -mavx2, which takes the source's
 * __FP_FAST_FMA branches and where the compiler contracted every product whose only uses are sums in its own basic block.  For y = 2 and x >= 0 the
 * sequence below is that variant's published algorithm, operation for operation and fused where it is fused there:
 *
 *   x = 0, inf, NaN                      x * x
 *   x subnormal                          scaled by 2^52, exponent corrected by -52
 *   x = 2^k z, z in [OFF, 2 OFF)         row i of the log table from the top 7 mantissa bits of (bits(x) - OFF)
 *   r = z invc - 1 (one FMA, exact)      hi + lo = k ln2 + log c + r - r^2 / 2 + r^3 P(r), the tail carried in lo
 *   ehi = 2 hi, elo = 2 lo (exact)       |ehi| < 2^-54: 1;  |ehi| >= 1024: overflow (inf) or underflow (0)
 *   kd = round(ehi N / ln2), r = ehi - kd ln2 / N + elo;  2^(kd / N) = scale (1 + tail) from the exp table
 *   result = scale + scale (tail + r + r^2 Q(r)), rescaled in two steps when |ehi| >= 512 (specialcase: results near the
 *   overflow threshold and in the subnormal range)
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' below is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add.  tests/test_pow2.py checks the host build of this file against libm pow(x, 2.0) bit for bit on > 10^7
 * arguments, and the device build against the host build.
 */
#ifndef D2D_POW2_H
#define D2D_POW2_H

#ifndef D2D_POW2_QUAL
#define D2D_POW2_QUAL static inline
#endif
#ifndef D2D_POW2_TBL_QUAL
#define D2D_POW2_TBL_QUAL static const
#endif
#ifndef D2D_FMA
#define D2D_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

#include "d2d_pow2_tbl.h"

D2D_POW2_QUAL double d2d_pow2_from_bits(unsigned long long b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}
D2D_POW2_QUAL unsigned long long d2d_pow2_bits(double d) {
  unsigned long long b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}

/* exp_inline's specialcase: scale's exponent would leave the double range, so it is applied in two steps */
D2D_POW2_QUAL double d2d_pow2_exp_special(double tmp, unsigned long long sbits, unsigned long long ki) {
  if ((ki & 0x80000000ull) == 0) {                      /* k > 0 */
    sbits -= 1009ull << 52;
    const double scale = d2d_pow2_from_bits(sbits);
    return 0x1p1009 * D2D_FMA(scale, tmp, scale);
  }
  sbits += 1022ull << 52;                               /* k < 0: care in the subnormal range */
  const double scale = d2d_pow2_from_bits(sbits);
  const double st = scale * tmp;                        /* one product with a use on either side of the branch: not fused there */
  double y = scale + st;
  if (__builtin_fabs(y) < 1.0) {
    double one = 1.0;
    if (y < 0.0) one = -1.0;
    double lo = (scale - y) + st;
    const double hi = one + y;
    lo = ((one - hi) + y) + lo;
    y = (hi + lo) - one;
    if (y == 0.0) y = d2d_pow2_from_bits(sbits & 0x8000000000000000ull);
  }
  return 0x1p-1022 * y;
}

/* libm pow(x, 2.0); the exponent is an even integer, so pow drops the sign of x before anything else */
D2D_POW2_QUAL double d2d_pow2(double x) {
  unsigned long long ix = d2d_pow2_bits(x) & 0x7fffffffffffffffull;
  const unsigned top = (unsigned)(ix >> 52);
  if (top - 1u >= 0x7feu) {                             /* zero, subnormal, inf, NaN */
    if (2 * ix == 0 || 2 * ix >= 2 * 0x7ff0000000000000ull) return x * x;
    ix = d2d_pow2_bits(x * 0x1p52) & 0x7fffffffffffffffull;   /* normalise a subnormal x */
    ix -= 52ull << 52;
  }
  /* ---- log_inline ---- */
  const double *LC = d2d_pow2_log_c;                    /* ln2hi, ln2lo, A[0..6] */
  const unsigned long long tmp = ix - 0x3fe6955500000000ull;
  const int i = (int)((tmp >> 45) & (D2D_POW2_N - 1));
  const int k = (int)((long long)tmp >> 52);
  const double z = d2d_pow2_from_bits(ix - (tmp & (0xfffull << 52)));
  const double kd = (double)k;
  const double invc = d2d_pow2_log_tbl[i][0], logc = d2d_pow2_log_tbl[i][1], logctail = d2d_pow2_log_tbl[i][2];
  const double r = D2D_FMA(z, invc, -1.0);
  const double t1 = D2D_FMA(kd, LC[0], logc);
  const double t2 = t1 + r;
  const double lo1 = D2D_FMA(kd, LC[1], logctail);
  const double lo2 = (t1 - t2) + r;
  const double ar = LC[2] * r;
  const double ar2 = r * ar;
  const double ar3 = r * ar2;
  const double lhi = t2 + ar2;
  const double lo3 = D2D_FMA(ar, r, -ar2);
  const double lo4 = (t2 - lhi) + ar2;
  const double p = ar3 * D2D_FMA(ar2, D2D_FMA(ar2, D2D_FMA(r, LC[8], LC[7]), D2D_FMA(r, LC[6], LC[5])), D2D_FMA(r, LC[4], LC[3]));
  const double llo = (((lo1 + lo2) + lo3) + lo4) + p;
  const double hi = lhi + llo;
  const double lo = (lhi - hi) + llo;
  /* ---- y = 2: both products are exact ---- */
  const double ehi = 2.0 * hi;
  const double elo = D2D_FMA(2.0, lo, D2D_FMA(2.0, hi, -ehi));
  /* ---- exp_inline ---- */
  const double *EC = d2d_pow2_exp_c;                    /* invln2N, shift, negln2hiN, negln2loN, C2..C5 */
  unsigned abstop = (unsigned)(d2d_pow2_bits(ehi) >> 52) & 0x7ffu;
  if (abstop - 0x3c9u >= 0x408u - 0x3c9u) {             /* |ehi| < 2^-54 or >= 512 */
    if (abstop - 0x3c9u >= 0x80000000u) return 1.0 + ehi;
    if (abstop >= 0x409u) return (d2d_pow2_bits(ehi) >> 63) ? 0x1p-767 * 0x1p-767 : 0x1p769 * 0x1p769;
    abstop = 0;
  }
  double kk = D2D_FMA(EC[0], ehi, EC[1]);
  const unsigned long long ki = d2d_pow2_bits(kk);
  kk -= EC[1];
  double rr = D2D_FMA(kk, EC[3], D2D_FMA(kk, EC[2], ehi));
  rr += elo;
  const unsigned idx = (unsigned)(ki & (D2D_POW2_N - 1));
  const unsigned long long etop = ki << 45;
  const double tail = d2d_pow2_from_bits(d2d_pow2_exp_tbl[idx][0]);
  const unsigned long long sbits = d2d_pow2_exp_tbl[idx][1] + etop;
  const double r2 = rr * rr;
  const double t = D2D_FMA(r2 * r2, D2D_FMA(rr, EC[7], EC[6]), D2D_FMA(r2, D2D_FMA(rr, EC[5], EC[4]), tail + rr));
  if (abstop == 0) return d2d_pow2_exp_special(t, sbits, ki);
  const double scale = d2d_pow2_from_bits(sbits);
  return D2D_FMA(scale, t, scale);
}

#endif /* D2D_POW2_H */
