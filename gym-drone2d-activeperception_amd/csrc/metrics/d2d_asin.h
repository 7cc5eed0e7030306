/*
 * d2d_asin.h — restatement of the host libm's asin, which Python's math.asin passes every argument of [-1, 1] to.
 *
 * Reference call sites: vo_calculator.py:87 `half_angle = math.asin((rA + rB) / dist)` (the velocity-obstacle cone's half angle;
 * the cone's edges are then compared with other angles, so the device has to return libm's bits, not just an accurate angle) and
 * utils.py:327, :346, :423 (the RVO motion profile: csrc/rvo/d2d_rvo.h includes this file unchanged).
 *
 * math.asin (CPython Modules/mathmodule.c, math_1 over libm's asin) returns NaN for NaN and RAISES ValueError for |x| > 1, where
 * libm returns NaN; d2d_asin returns libm's NaN there.  The velocity-obstacle caller never passes such a value (d2d_vo_half).
 *
 * The reference's runtime links glibc 2.35, whose double asin is the IBM Accurate Mathematical Library routine
 * (sysdeps/ieee754/dbl-64/e_asin.c + asincos.tbl + root.tbl, LGPL-2.1-or-later) with the multi-precision slow paths removed
 * (glibc 2.34): the first-stage result is returned, so it is NOT correctly rounded and an accurate device asin does not match it.
 * x86-64 libm dispatches asin through an ifunc; on every CPU with FMA it resolves to the variant built with -mfma, where the
 * compiler contracted a fixed set of multiply-adds.  The sequence below is that variant's published algorithm, operation for
 * operation and fused where it is fused there.  With m the high word of x as a signed int and k = m & 0x7fffffff:
 *
 *   k <  0x3e500000  (|x| < 2^-26)        x
 *   k <  0x3fc00000  (|x| < 1/8)          x + x^3 P(x^2), P = f1 .. f6 by Horner
 *   k <  0x3fef0000  (|x| < 31/32)        the row of asincos.tbl whose bucket holds |x| (width 2^-8; 11 doubles a row below 1/2,
 *                                         then 12, 13, 14, 15 as the polynomial grows towards 1): with xx = |x| - x_i,
 *                                         asin x_i + (xx / sqrt(1 - x_i^2) + (xx^2 Q(xx) + low part of asin x_i)), Q = c2 .. ch
 *   k <  0x3ff00000  (|x| < 1)            pi/2 - 2 asin(sqrt(z)), z = (1 - |x|) / 2: 1 / sqrt(z) from a seed of root.tbl, one
 *                                         polynomial and one Newton step; sqrt(z) = y + cc with y rounded to 29 bits; the
 *                                         polynomial P again; pi/2 as the double-length hp0 + hp1
 *   |x| == 1                              +-hp0
 *   otherwise (|x| > 1, NaN)              NaN
 *   each result takes the sign of x.
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' below is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add.  tests/test_asin.py checks the host build of this file against libm's asin / math.asin bit for bit on > 10^7
 * arguments, tests/test_gpu_asin.py the device build.
 */
#ifndef D2D_ASIN_H
#define D2D_ASIN_H

#ifndef D2D_ASIN_QUAL
#define D2D_ASIN_QUAL static inline
#endif
#ifndef D2D_ASIN_TBL_QUAL
#define D2D_ASIN_TBL_QUAL static const
#endif
#ifndef D2D_FMA
#define D2D_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

#include "d2d_asin_tbl.h"

/* P(v) = f1 + v (f2 + ... v f6): the Taylor tail of asin, (asin x - x) / x^3 at v = x^2 */
D2D_ASIN_QUAL double d2d_asin_poly(double v) {
  const double f6 = 0x1.292d80f453c72p-6, f5 = 0x1.6e442c822d419p-6, f4 = 0x1.f1c7e04f4ad99p-6, f3 = 0x1.6db6dae42c0e4p-5,
               f2 = 0x1.333333336127dp-4, f1 = 0x1.55555555554f9p-3;
  double p = D2D_FMA(v, f6, f5);
  p = D2D_FMA(v, p, f4);
  p = D2D_FMA(v, p, f3);
  p = D2D_FMA(v, p, f2);
  return D2D_FMA(v, p, f1);
}

/* the table branches: row T[n ..], top coefficient T[n + h]; ax = |x| */
D2D_ASIN_QUAL double d2d_asin_row(double ax, int n, int h) {
  const double *T = d2d_asin_tbl + n;
  const double xx = ax - T[0];
  double q = T[h];
  for (int i = h - 1; i >= 2; --i) q = D2D_FMA(xx, q, T[i]);
  const double p = D2D_FMA(xx * xx, q, T[h + 1]);
  const double t = D2D_FMA(T[1], xx, p);
  return T[h + 2] + t;
}

/* libm's asin */
D2D_ASIN_QUAL double d2d_asin(double x) {
  const double hp0 = 0x1.921fb54442d18p+0, hp1 = 0x1.1a62633145c07p-54;
  const double rt3 = 0x1.4006318d1dab9p-2, rt2 = 0x1.800496769c91ap-2, rt1 = 0x1.fffffff757304p-2, rt0 = 0x1.fffffffecc1ddp-1;
  const double t24 = 0x1p24;
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  const int m = (int)(unsigned)(b >> 32);
  const int k = m & 0x7fffffff;
  const double ax = (m > 0) ? x : -x;
  double res;

  if (k < 0x3e500000) return x;
  if (k < 0x3fc00000) {
    const double x2 = x * x;
    return D2D_FMA(d2d_asin_poly(x2), x2 * x, x);
  }
  if (k < 0x3fd00000) res = d2d_asin_row(ax, 11 * ((k & 0xfffff) >> 15), 6);
  else if (k < 0x3fe00000) res = d2d_asin_row(ax, 11 * ((k & 0xfffff) >> 14) + 352, 6);
  else if (k < 0x3fe80000) res = d2d_asin_row(ax, 1056 + 12 * ((k & 0xfe000) >> 13), 7);
  else if (k < 0x3fed8000) res = d2d_asin_row(ax, 992 + 13 * ((k & 0xfe000) >> 13), 8);
  else if (k < 0x3fee8000) res = d2d_asin_row(ax, 884 + 14 * ((k & 0xfe000) >> 13), 9);
  else if (k < 0x3fef0000) res = d2d_asin_row(ax, 768 + 15 * ((k & 0xfe000) >> 13), 10);
  else if (k < 0x3ff00000) {
    const double z = 0.5 * ((m > 0) ? (1.0 - x) : (1.0 + x));
    unsigned long long bz;
    __builtin_memcpy(&bz, &z, 8);
    const int kk = (int)(unsigned)(bz >> 32);
    const unsigned long long bp = (unsigned long long)(1023 + 511 - (kk >> 21)) << 52;   /* 2^(511 - (kk >> 21)): 2^3 .. 2^27 */
    double pw;
    __builtin_memcpy(&pw, &bp, 8);
    double t = d2d_asin_inroot[(kk & 0x001fffff) >> 14] * pw;
    const double r = D2D_FMA(-(t * t), z, 1.0);
    t = t * D2D_FMA(r, D2D_FMA(r, D2D_FMA(r, rt3, rt2), rt1), rt0);
    const double c = t * z;
    t = c * D2D_FMA(-(0.5 * t), c, 1.5);
    const double y = (c + t24) - t24;
    const double cc = D2D_FMA(-y, y, z) / (t + y);
    const double p = d2d_asin_poly(z) * z;
    const double cor = D2D_FMA(-(2.0 * (y + cc)), p, D2D_FMA(-2.0, cc, hp1));
    const double res1 = D2D_FMA(-2.0, y, hp0);
    res = res1 + cor;
  } else if (k == 0x3ff00000 && (unsigned)b == 0u) {
    res = hp0;
  } else {
    return __builtin_nan("");
  }
  return (m > 0) ? res : -res;
}

#endif /* D2D_ASIN_H */
