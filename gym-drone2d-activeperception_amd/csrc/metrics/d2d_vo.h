/*
 * d2d_vo.h — per-element arithmetic of the velocity-obstacle feasibility metric (include/d2d_metrics.h names the reference lines).
 *
 * The reference (script/difficulty_calculator/vo_calculator.py) evaluates, for a drone of radius rA at position pA and agent j
 * (position pB, preferred velocity vB, radius rB):
 *
 *   dist      = numpy.linalg.norm(pA - pB)            a 2-vector: sqrt(dot), and numpy's dot of two elements is
 *                                                      fma(y, y, x * x) with x = pA.x - pB.x, y = pA.y - pB.y
 *   theta_BA  = math.atan2(pB.y - pA.y, pB.x - pA.x)
 *   collided  = dist < rA + rB
 *   arg       = (rA + rB) / dist
 *   half      = math.asin(arg)                        the cone's half angle: d2d_asin.h on the device, or the host's libm
 *   left      = math.atan2(sin(theta_BA + half), cos(theta_BA + half))
 *   right     = math.atan2(sin(theta_BA - half), cos(theta_BA - half))
 *   theta_dif = math.atan2(v.y - vB.y, v.x - vB.x)    per (candidate velocity v, agent): no position in it
 *   in_between(right, theta_dif, left)                 with the script's 3.14 and 2 * 3.14
 *
 * The scalar pieces below are shared by the device kernels (d2d_metrics.hip) and by the plain array loops at the end of this file
 * (host builds only), which the CPU tests compare with a Python model bit for bit.
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add (the one inside numpy's norm).
 */
#ifndef D2D_VO_IMPL_H
#define D2D_VO_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d.h" /* D2D_AF, D2D_A_*: the rows of the state's agents [6][N] */
#include "../../../include/d2d_metrics.h"

#ifndef D2D_VO_QUAL
#define D2D_VO_QUAL static inline
#endif
#ifndef D2D_SINCOS_QUAL
#define D2D_SINCOS_QUAL D2D_VO_QUAL
#endif
#ifndef D2D_ATAN2_QUAL
#define D2D_ATAN2_QUAL D2D_VO_QUAL
#endif
#ifndef D2D_ASIN_QUAL
#define D2D_ASIN_QUAL D2D_VO_QUAL
#endif
#include "../d2d_atan2.h"
#include "../d2d_sincos.h"
#include "d2d_asin.h"

/* numpy.linalg.norm of the 2-vector (x, y) */
D2D_VO_QUAL double d2d_vo_norm(double x, double y) { return __builtin_sqrt(D2D_FMA(y, y, x * x)); }

/* vo_calculator.py:80-83: dist, theta_BA and the collision test of one (position, agent); returns dist < rA + rB */
D2D_VO_QUAL int d2d_vo_pair(double ax, double ay, double bx, double by, double rA, double rB, double *arg, double *theta_ba) {
  const double dist = d2d_vo_norm(ax - bx, ay - by);
  const double rr = rA + rB;
  *theta_ba = d2d_atan2(by - ay, bx - ax);
  *arg = rr / dist;
  return dist < rr;
}

/* the collision test alone */
D2D_VO_QUAL int d2d_vo_hits(double ax, double ay, double bx, double by, double rA, double rB) {
  return d2d_vo_norm(ax - bx, ay - by) < rA + rB;
}

/* vo_calculator.py:87: the half angle of one pair.  arg > 1 only for a pair that touches, whose position is in collision: the
 * reference never evaluates it (math.asin would raise), the host path (metrics.host_asin) writes 0 there and so does this. */
D2D_VO_QUAL double d2d_vo_half(double arg) { return arg > 1.0 ? 0.0 : d2d_asin(arg); }

/* vo_calculator.py:88-91 and :107-108: the cone's edges as the script's atan2 of (sin, cos) returns them */
D2D_VO_QUAL void d2d_vo_cone(double theta_ba, double half, double *right, double *left) {
  const double l = theta_ba + half, r = theta_ba - half;
  *left = d2d_atan2(d2d_sin(l), d2d_cos(l));
  *right = d2d_atan2(d2d_sin(r), d2d_cos(r));
}

/* vo_calculator.py:106 */
D2D_VO_QUAL double d2d_vo_theta_dif(double cx, double cy, double vbx, double vby) { return d2d_atan2(cy - vby, cx - vbx); }

/* vo_calculator.py:10-33, branch for branch */
D2D_VO_QUAL int d2d_vo_in_between(double right, double dif, double left) {
  if (__builtin_fabs(right - left) <= 3.14) return right <= dif && dif <= left;
  if (left < 0.0 && right > 0.0) {
    left += 2 * 3.14;
    if (dif < 0.0) dif += 2 * 3.14;
    return right <= dif && dif <= left;
  }
  if (left > 0.0 && right < 0.0) {
    right += 2 * 3.14;
    if (dif < 0.0) dif += 2 * 3.14;
    return left <= dif && dif <= right;
  }
  return 0;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- the entry points as plain loops over host arrays (tests/csrc/vo_host.c), same layouts as include/d2d_metrics.h ---- */

D2D_VO_QUAL void d2d_vo_geometry_seq(const double *agents, const double *pos, double rA, int B, int N, int P, double *arg,
                                     double *theta_ba, uint8_t *collided) {
  for (int b = 0; b < B; ++b) {
    const double *ag = agents + (size_t)b * D2D_AF * N;
    for (int p = 0; p < P; ++p) {
      int hit = 0;
      for (int j = 0; j < N; ++j) {
        const size_t o = ((size_t)b * P + p) * N + j;
        hit |= d2d_vo_pair(pos[2 * p], pos[2 * p + 1], ag[D2D_A_PX * N + j], ag[D2D_A_PY * N + j], rA, ag[D2D_A_R * N + j],
                           arg + o, theta_ba + o);
      }
      collided[(size_t)b * P + p] = (uint8_t)hit;
    }
  }
}

D2D_VO_QUAL void d2d_vo_cones_seq(const double *theta_ba, const double *half, const uint8_t *collided, int B, int N, int P,
                                  double *cone) {
  for (size_t bp = 0; bp < (size_t)B * P; ++bp)
    for (int j = 0; j < N; ++j) {
      const size_t o = bp * N + j;
      cone[2 * o] = cone[2 * o + 1] = 0.0;
      if (!collided[bp]) d2d_vo_cone(theta_ba[o], half[o], cone + 2 * o, cone + 2 * o + 1);
    }
}

/* d2d_vo_cones_arg: the half angle taken here; half_out may be NULL */
D2D_VO_QUAL void d2d_vo_cones_arg_seq(const double *theta_ba, const double *arg, const uint8_t *collided, int B, int N, int P,
                                      double *half_out, double *cone) {
  for (size_t bp = 0; bp < (size_t)B * P; ++bp)
    for (int j = 0; j < N; ++j) {
      const size_t o = bp * N + j;
      const double half = d2d_vo_half(arg[o]);
      if (half_out) half_out[o] = half;
      cone[2 * o] = cone[2 * o + 1] = 0.0;
      if (!collided[bp]) d2d_vo_cone(theta_ba[o], half, cone + 2 * o, cone + 2 * o + 1);
    }
}

D2D_VO_QUAL void d2d_vo_count_seq(const double *agents, const double *cand, const double *cone, const uint8_t *collided, int B,
                                  int N, int P, int C, int32_t *count) {
  for (int b = 0; b < B; ++b) {
    const double *ag = agents + (size_t)b * D2D_AF * N;
    for (int p = 0; p < P; ++p) {
      const size_t bp = (size_t)b * P + p;
      if (collided[bp]) {
        count[bp] = -1;
        continue;
      }
      int32_t n = 0;
      for (int c = 0; c < C; ++c) {
        int suit = 1;
        for (int j = 0; j < N && suit; ++j) {
          const double dif = d2d_vo_theta_dif(cand[2 * c], cand[2 * c + 1], ag[D2D_A_VX * N + j], ag[D2D_A_VY * N + j]);
          if (d2d_vo_in_between(cone[2 * (bp * N + j)], dif, cone[2 * (bp * N + j) + 1])) suit = 0;
        }
        n += suit;
      }
      count[bp] = n;
    }
  }
}
#endif

#endif /* D2D_VO_IMPL_H */
