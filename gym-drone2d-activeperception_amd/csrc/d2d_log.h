/*
 * d2d_log.h — restatement of the libm log(x) that the reference's measurement noise calls.
 *
 * Reference call site: utils.py:605 `np.random.randn(2)`.  numpy's legacy Gaussian (the polar method over MT19937) evaluates
 * f = sqrt(-2.0 * log(r2) / r2) with the host libm's log, and the measurement that carries f feeds a Kalman filter whose
 * state is compared bit for bit, so the device has to return libm's bits.
 *
 * glibc 2.35's double log (sysdeps/ieee754/dbl-64/e_log.c, from the ARM optimized routines, MIT / LGPL-2.1-or-later) has two
 * paths: a degree-11 polynomial in r = x - 1 for x in [1 - 2^-4, 1 + 0x1.09p-4), whose leading terms r - r^2 / 2 are carried as
 * hi + lo with r split at 2^27; and, elsewhere, x = 2^k z with z in [OFF, 2 OFF), a 128-row table (__log_data) of invc ~ 1 / c,
 * logc ~ log c for c near the centre of z's subinterval, and a degree-5 polynomial in r = z invc - 1.  x86-64 libm dispatches
 * log through an ifunc; on every CPU with FMA + AVX2 it resolves to the variant built with -mfma -mavx2, which takes the
 * source's __FP_FAST_FMA branch and where the compiler contracted the products that feed a sum.  The sequence below is that
 * variant's published algorithm, operation for operation and fused where it is fused there (note r 2^27, formed twice, each
 * time inside an FMA: rhi = (r + r 2^27) - r 2^27 with one rounding per line).
 *
 *   x = 1                                +0
 *   x = +-0                              -inf;  x = +inf: +inf;  x < 0, NaN: NaN
 *   x subnormal                          scaled by 2^52, exponent corrected by -52
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' below is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add.  tests/test_log.py checks the host build of this file against libm log bit for bit on > 10^7 arguments, and
 * the device build against the host build.
 */
#ifndef D2D_LOG_H
#define D2D_LOG_H

#ifndef D2D_LOG_QUAL
#define D2D_LOG_QUAL static inline
#endif
#ifndef D2D_LOG_TBL_QUAL
#define D2D_LOG_TBL_QUAL static const
#endif
#ifndef D2D_FMA
#define D2D_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

#include "d2d_log_tbl.h"

D2D_LOG_QUAL double d2d_log_from_bits(unsigned long long b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}
D2D_LOG_QUAL unsigned long long d2d_log_bits(double d) {
  unsigned long long b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}

/* libm log(x) */
D2D_LOG_QUAL double d2d_log(double x) {
  const double *LC = d2d_log_c;                         /* ln2hi, ln2lo, A[0..4], B[0..10] */
  const double *A = LC + 2, *B = LC + 7;
  unsigned long long ix = d2d_log_bits(x);
  const unsigned top = (unsigned)(ix >> 48);
  if (ix - 0x3fee000000000000ull < 0x3ff1090000000000ull - 0x3fee000000000000ull) {   /* 1 - 2^-4 <= x < 1 + 0x1.09p-4 */
    if (ix == 0x3ff0000000000000ull) return 0.0;
    const double r = x - 1.0;
    const double r2 = r * r;
    const double r3 = r * r2;
    const double q3 = D2D_FMA(r3, B[10], D2D_FMA(r2, B[9], D2D_FMA(r, B[8], B[7])));
    const double q2 = D2D_FMA(r2, B[6], D2D_FMA(r, B[5], B[4]));
    const double q1 = D2D_FMA(r2, B[3], D2D_FMA(r, B[2], B[1]));
    const double p = D2D_FMA(D2D_FMA(q3, r3, q2), r3, q1);
    const double t = D2D_FMA(r, 0x1p27, r);
    const double rhi = D2D_FMA(-0x1p27, r, t);
    const double rlo = r - rhi;
    const double s = rhi * rhi;
    const double hi = D2D_FMA(s, B[0], r);
    double lo = D2D_FMA(s, B[0], r - hi);
    lo = D2D_FMA(B[0] * rlo, r + rhi, lo);
    return hi + D2D_FMA(p, r3, lo);
  }
  if (top - 0x0010u >= 0x7ff0u - 0x0010u) {             /* x < 2^-1022, inf or NaN */
    if (ix * 2 == 0) return -1.0 / 0.0;
    if (ix == 0x7ff0000000000000ull) return x;
    if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) return (x - x) / (x - x);
    ix = d2d_log_bits(x * 0x1p52);                      /* normalise a subnormal x */
    ix -= 52ull << 52;
  }
  const unsigned long long tmp = ix - 0x3fe6000000000000ull;
  const int i = (int)((tmp >> 45) & (D2D_LOG_N - 1));
  const int k = (int)((long long)tmp >> 52);
  const double z = d2d_log_from_bits(ix - (tmp & (0xfffull << 52)));
  const double invc = d2d_log_tbl[i][0], logc = d2d_log_tbl[i][1];
  const double r = D2D_FMA(z, invc, -1.0);
  const double kd = (double)k;
  const double w = D2D_FMA(kd, LC[0], logc);
  const double hi = w + r;
  const double lo = D2D_FMA(kd, LC[1], (w - hi) + r);
  const double r2 = r * r;
  const double r3 = r * r2;
  const double p = D2D_FMA(D2D_FMA(r, A[4], A[3]), r2, D2D_FMA(r, A[2], A[1]));
  return D2D_FMA(r3, p, D2D_FMA(r2, A[0], lo)) + hi;
}

#endif /* D2D_LOG_H */
