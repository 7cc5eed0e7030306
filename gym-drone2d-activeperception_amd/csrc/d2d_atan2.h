/*
 * d2d_atan2.h — restatement of Python's math.atan2 (CPython m_atan2 over the host libm atan2) that the
 * reference's LookAhead and LookGoal gaze policies call.
 *
 * Reference call sites: yaw_planner.py:33 `math.atan2(-vy, vx)` (LookAhead) and yaw_planner.py:251
 * `math.atan2(-(ly - y), lx - x)` (LookGoal); the heading in degrees is then compared with the yaw, so
 * the device has to return libm's bits, not just an accurate angle.
 *
 * CPython's m_atan2 (Modules/mathmodule.c) decides the special cases itself:
 *   NaN in                               NaN
 *   y = +-inf                            +-pi/4, +-3pi/4 (x = +inf, -inf) or +-pi/2 (x finite)
 *   x = +-inf or y == 0                  copysign(0, y) for sign(x) = +, copysign(pi, y) for sign(x) = -
 *                                        (atan2(-0.0, 0.0) = -0.0 occurs in the reference's LookGoal)
 * and only then calls libm.  The reference's runtime links glibc 2.35, whose double atan2 is the IBM Accurate
 * Mathematical Library routine (sysdeps/ieee754/dbl-64/e_atan2.c + uatan2.tbl, LGPL-2.1-or-later) with
 * the multi-precision slow paths removed (glibc 2.34): the first-stage result is returned, so it is NOT
 * correctly rounded and an accurate device atan2 does not match it.  x86-64 libm dispatches atan2 through
 * an ifunc; on every CPU with FMA + AVX2 it resolves to the variant built with -mfma -mavx2, where the
 * compiler contracted a fixed set of multiply-adds.  For finite x, finite y != 0 the sequence below is
 * that variant's published algorithm, operation for operation and fused where it is fused there:
 *
 *   x == 0                               +-pi/2 by the sign of y
 *   de = exponent(y) - exponent(x)       de >= 57: +-pi/2 by y > 0;  de <= -57: x > 0 ? copysign(ay / ax, y)
 *                                        : +-pi by y > 0
 *   ax, ay scaled by 2^+-500 when one of them lies below 2^-500 or above 2^500
 *   u + du = min / max of ax, ay         u rounded, du = (num - u * den exactly) / den (EMULV by an FMA)
 *   (i)   x > 0, ay <  ax   atan u       u < 1/16: u + fma(u v, P(v), du), v = u^2, P = d3..d13
 *                                        else row i = round(256 u) - 16 of the table (x_i, atan x_i,
 *                                        1 / (1 + x_i^2), c3..c6): t1 + (v t2 + (dv t2 + v^2 Q(v)))
 *   (ii)  x > 0, ay >= ax   pi/2 - atan u
 *   (iii) x < 0, ax <  ay   pi/2 + atan u
 *   (iv)  x < 0, ay <= ax   pi - atan u  (pi/2 and pi as double-length hpi + hpi1, opi + opi1)
 *   each result takes the sign of y.
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' below is one IEEE-754 binary64
 * operation, every D2D_FMA one fused multiply-add.  tests/test_atan2.py checks the host build of this file
 * against math.atan2 / libm atan2 bit for bit on > 10^7 pairs, tests/test_gpu_heading_gaze.py the device
 * build.
 */
#ifndef D2D_ATAN2_H
#define D2D_ATAN2_H

#ifndef D2D_ATAN2_QUAL
#define D2D_ATAN2_QUAL static inline
#endif
#ifndef D2D_ATAN2_TBL_QUAL
#define D2D_ATAN2_TBL_QUAL static const
#endif
#ifndef D2D_FMA
#define D2D_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

#include "d2d_atan2_tbl.h"

/* glibc's EADD / ESUB (dla.h): z + zz = x + y and x - y as double-length sums */
#define D2D_ATAN2_EADD(x, y, z, zz) do { z = (x) + (y); \
  zz = (__builtin_fabs(x) > __builtin_fabs(y)) ? (((x) - z) + (y)) : (((y) - z) + (x)); } while (0)
#define D2D_ATAN2_ESUB(x, y, z, zz) do { z = (x) - (y); \
  zz = (__builtin_fabs(x) > __builtin_fabs(y)) ? (((x) - z) - (y)) : ((x) - ((y) + z)); } while (0)

/* libm atan2 for finite x, finite y != 0 (the calls m_atan2 passes on) */
D2D_ATAN2_QUAL double d2d_atan2_finite(double y, double x) {
  const double hpi = 0x1.921fb54442d18p+0, hpi1 = 0x1.1a62633145c07p-54;
  const double opi = 0x1.921fb54442d18p+1, opi1 = 0x1.1a62633145c07p-53;
  const double inv16 = 0x1p-4, two8 = 0x1p+8, two52 = 0x1p+52, two500 = 0x1p+500, twom500 = 0x1p-500;
  const double d3 = -0x1.5555555555555p-2, d5 = 0x1.99999999997fdp-3, d7 = -0x1.24924923f7603p-3,
               d9 = 0x1.c71c6e5129a3bp-4, d11 = -0x1.7458022b13c25p-4, d13 = 0x1.375f08b31cbcep-4;

  if (x == 0.0) return __builtin_signbit(y) ? -hpi : hpi;
  unsigned long long bx, by;
  __builtin_memcpy(&bx, &x, 8);
  __builtin_memcpy(&by, &y, 8);
  const int de = (int)((by >> 32) & 0x7ff00000u) - (int)((bx >> 32) & 0x7ff00000u);
  if (de >= 59768832) return (y > 0.0) ? hpi : -hpi;            /* 57 * 16^5 */
  if (de <= -59768832) {
    if (x > 0.0) return __builtin_copysign(__builtin_fabs(y) / __builtin_fabs(x), y);
    return (y > 0.0) ? opi : -opi;
  }

  double ax = (x < 0.0) ? -x : x, ay = (y < 0.0) ? -y : y;
  if (ax < twom500 || ay < twom500) { ax *= two500; ay *= two500; }
  if (ax > two500 || ay > two500) { ax *= twom500; ay *= twom500; }

  double u, du;
  if (ay < ax) {
    u = ay / ax;
    const double v = ax * u, vv = D2D_FMA(ax, u, -v);
    du = ((ay - v) - vv) / ax;
  } else {
    u = ax / ay;
    const double v = ay * u, vv = D2D_FMA(ay, u, -v);
    du = ((ax - v) - vv) / ay;
  }

  double z;
  if (u < inv16) {
    const double v = u * u;
    double p = D2D_FMA(v, d13, d11);
    p = D2D_FMA(v, p, d9);
    p = D2D_FMA(v, p, d7);
    p = D2D_FMA(v, p, d5);
    p = D2D_FMA(v, p, d3);
    if (x > 0.0 && ay < ax) {                                    /* (i) */
      z = u + D2D_FMA(u * v, p, du);
    } else {
      const double zz = (u * v) * p;
      double t2, cor;
      if (x > 0.0) {                                             /* (ii) */
        D2D_ATAN2_ESUB(hpi, u, t2, cor);
        z = t2 + (((hpi1 + cor) - du) - zz);
      } else if (ax < ay) {                                      /* (iii) */
        D2D_ATAN2_EADD(hpi, u, t2, cor);
        z = t2 + (((hpi1 + cor) + du) + zz);
      } else {                                                   /* (iv) */
        D2D_ATAN2_ESUB(opi, u, t2, cor);
        z = t2 + (((opi1 + cor) - du) - zz);
      }
    }
  } else {
    const int i = (int)(D2D_FMA(u, two8, two52) - two52) - 16;
    const double *c = d2d_atan2_tbl[i];
    if (x > 0.0 && ay < ax) {                                    /* (i) */
      const double t3 = u - c[0];
      double v, dv;
      D2D_ATAN2_EADD(t3, du, v, dv);
      double q = D2D_FMA(v, c[6], c[5]);
      q = D2D_FMA(v, q, c[4]);
      q = D2D_FMA(v, q, c[3]);
      const double zz = D2D_FMA(v, c[2], D2D_FMA(dv, c[2], (v * v) * q));
      z = c[1] + zz;
    } else {
      const double v = (u - c[0]) + du;
      double q = D2D_FMA(v, c[6], c[5]);
      q = D2D_FMA(v, q, c[4]);
      q = D2D_FMA(v, q, c[3]);
      q = D2D_FMA(v, q, c[2]);
      if (x > 0.0) z = (hpi - c[1]) + D2D_FMA(-v, q, hpi1);     /* (ii) */
      else if (ax < ay) z = (hpi + c[1]) + D2D_FMA(v, q, hpi1); /* (iii) */
      else z = (opi - c[1]) + D2D_FMA(-v, q, opi1);             /* (iv) */
    }
  }
  return __builtin_copysign(z, y);
}

/* Python's math.atan2(y, x) */
D2D_ATAN2_QUAL double d2d_atan2(double y, double x) {
  const double pi = 0x1.921fb54442d18p+1;
  if (__builtin_isnan(x) || __builtin_isnan(y)) return __builtin_nan("");
  if (__builtin_isinf(y)) {
    if (__builtin_isinf(x)) return __builtin_copysign(__builtin_signbit(x) ? 0.75 * pi : 0.25 * pi, y);
    return __builtin_copysign(0.5 * pi, y);
  }
  if (__builtin_isinf(x) || y == 0.0) return __builtin_copysign(__builtin_signbit(x) ? pi : 0.0, y);
  return d2d_atan2_finite(y, x);
}

#endif /* D2D_ATAN2_H */
