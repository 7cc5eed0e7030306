/*
 * d2d_gaze.h — per-element arithmetic of the step path's gaze decision (include/d2d_gaze.h names the reference lines).
 *
 * LookAhead.plan (yaw_planner.py:28-39) and Owl.plan (:151-222) as IEEE-754 binary64 operations in the reference's own order:
 *   math.degrees(r)            r * (180 / pi), one multiplication
 *   math.radians(d)            d * (pi / 180), one multiplication
 *   a % 360                    Python's float modulo (d2d_gaze_mod360)
 *   math.atan2                 d2d_atan2 (../d2d_atan2.h), the host libm's bits
 *   x ** 2 on a numpy float64  libm's pow(x, 2.0): d2d_pow2 (../d2d_pow2.h)
 *   numpy's dot / norm of two  fma(b1, b2, a1 * a2) and its square root
 *   f[i, :].dot(lamb)          five FMAs from 0
 *   Python's min / max         the first argument unless the second compares smaller / larger: a NaN passes through
 *   np.minimum                 hands a NaN on
 *   np.argmin                  the first minimum; the first NaN wins outright
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one operation, every D2D_FMA one fused multiply-add.  The scalar
 * pieces are shared by the device kernels (d2d_gaze.hip) and by the plain loops at the end of this file (host builds only), which the
 * CPU tests compare with the package's host policies bit for bit.
 */
#ifndef D2D_GAZE_IMPL_H
#define D2D_GAZE_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_gaze.h"

#ifndef D2D_GAZE_QUAL
#define D2D_GAZE_QUAL static inline
#endif
#ifndef D2D_ATAN2_QUAL
#define D2D_ATAN2_QUAL D2D_GAZE_QUAL
#endif
#ifndef D2D_POW2_QUAL
#define D2D_POW2_QUAL D2D_GAZE_QUAL
#endif
#include "../d2d_atan2.h"
#include "../d2d_pow2.h"

#define D2D_GAZE_DF 8      /* doubles of one drone record: x, y, yaw, vx, vy (D2D_D_* of include/d2d.h) */
#define D2D_GAZE_KF 20     /* doubles of one Kalman record, mu first (D2D_KF) */
#define D2D_GAZE_F_DONE 3  /* D2D_F_DONE */
#define D2D_GAZE_NRATE 20  /* D2D_OWL_NRATE: len(Owl.u_space) */
#define D2D_GAZE_NDIR 36   /* D2D_OWL_NDIR: len(Owl.U_list) */
/* offsets into owl_tab: D2D_OWL_T_* of include/d2d.h */
#define D2D_GAZE_T_RATE 0
#define D2D_GAZE_T_RATE08 20
#define D2D_GAZE_T_TURN 40
#define D2D_GAZE_T_ACT 60
#define D2D_GAZE_T_DIR 80
#define D2D_GAZE_T_FOV 152
#define D2D_GAZE_T_DEPTH 153
#define D2D_GAZE_T_HOLD 154

#define D2D_GAZE_RAD2DEG 0x1.ca5dc1a63c1f8p+5 /* 180 / pi */
#define D2D_GAZE_DEG2RAD 0x1.1df46a2529d39p-6 /* pi / 180 */

/* numpy.linalg.norm of a 2-vector */
D2D_GAZE_QUAL double d2d_gaze_norm(double x, double y) { return __builtin_sqrt(D2D_FMA(y, y, x * x)); }

/* Python's float `a % 360.0` (py_mod360 of d2d_hip.hip, restated): the exact fmod without a loop, then the sign fix-up */
D2D_GAZE_QUAL double d2d_gaze_mod360(double a) {
  const double b = 360.0, fa = __builtin_fabs(a);
  const double n = __builtin_trunc(fa * 0x1.6c16c16c16c17p-9 /* 1 / 360 */);
  double m = D2D_FMA(-n, b, fa);
  if (m < 0.0) m = D2D_FMA(-(n - 1.0), b, fa);
  else if (m >= b) m = D2D_FMA(-(n + 1.0), b, fa);
  m = __builtin_copysign(m, a);
  if (m != 0.0) {
    if (m < 0.0) m += b;
  } else {
    m = 0.0;
  }
  return m;
}

/* LookAhead.plan for a drone with velocity (vx, vy) and yaw `yaw` (degrees); w = drone_max_yaw_speed */
D2D_GAZE_QUAL double d2d_gaze_lookahead(double vx, double vy, double yaw, double dt, double w) {
  if (vx == 0.0 && vy == 0.0) return 0.0;
  const double heading = d2d_gaze_mod360(d2d_atan2(-vy, vx) * D2D_GAZE_RAD2DEG);
  const double delta = heading - yaw;
  const double q = delta / dt, lo = (w < q) ? w : q, rate = (-w > lo) ? -w : lo;
  return (__builtin_fabs(delta) < 180.0 ? rate : -rate) / w;
}

/* angle_between (yaw_planner.py:144-149) of two angles already reduced % 360 */
D2D_GAZE_QUAL double d2d_gaze_apart(double am, double bm) {
  const double d = __builtin_fabs(am - bm), f = 360.0 - d;
  return (d < f) ? d : f;
}

/* Owl.G (:169-173): 0 inside the field of view, else the product of the angles (radians) to its two edges.  hp, hn: (fov / 2) % 360
 * and (-fov / 2) % 360.  A NaN direction fails the `<=` and comes back as NaN */
D2D_GAZE_QUAL double d2d_gaze_unseen(double theta, double half, double hp, double hn) {
  const double m = d2d_gaze_mod360(theta);
  if (d2d_gaze_apart(m, 0.0) <= half) return 0.0;
  return (d2d_gaze_apart(m, hp) * D2D_GAZE_DEG2RAD) * (d2d_gaze_apart(m, hn) * D2D_GAZE_DEG2RAD);
}

/* update_U (:175-181) of direction k: the new score.  ym: (-yaw) % 360 */
D2D_GAZE_QUAL double d2d_gaze_score(double old, int k, double vx, double vy, double ym, const double *tab, double half, double depth) {
  const double cs = tab[D2D_GAZE_T_DIR + 2 * k], sn = tab[D2D_GAZE_T_DIR + 2 * k + 1];
  const double mx = vx * 0.8, my = vy * 0.8;
  double g = -D2D_FMA(my, sn, mx * cs) / depth;
  g += (d2d_gaze_apart(10.0 * (double)k, ym) < half) ? 0.4 : -0.05;
  const double v = old + g;
  const double lo = (1.0 < v) ? 1.0 : v;
  return (0.0 > lo) ? 0.0 : lo;
}

/* U (:183-185): the index of the first of the 36 directions nearest to thm = theta % 360; a NaN answers 0 */
D2D_GAZE_QUAL int d2d_gaze_nearest(double thm) {
  int best = 0;
  double best_d = d2d_gaze_apart(0.0, thm);
  for (int k = 1; k < D2D_GAZE_NDIR; ++k) {
    const double a = d2d_gaze_apart(10.0 * (double)k, thm);
    if (a < best_d) {
      best = k;
      best_d = a;
    }
  }
  return best;
}

/* f[i, :].dot(lamb) (:217), lamb = [0.2, 0.9, 1, 0.1, 0] */
D2D_GAZE_QUAL double d2d_gaze_cost(double t0, double t1, double t2, double t3, double t4) {
  double cost = D2D_FMA(t0, 0.2, 0.0);
  cost = D2D_FMA(t1, 0.9, cost);
  cost = D2D_FMA(t2, 1.0, cost);
  cost = D2D_FMA(t3, 0.1, cost);
  return D2D_FMA(t4, 0.0, cost);
}

/* one step of np.argmin's walk: does `v` at a later index replace the best so far? */
D2D_GAZE_QUAL int d2d_gaze_better(double v, double best) { return best == best && (v < best || v != v); }

/* the direction (degrees) of tracker mean `ma` seen from (x0, y0), and the weight tracker `mj` gives (:197, beta = 1) */
D2D_GAZE_QUAL double d2d_gaze_agent_dir(const double *ma, double x0, double y0) {
  return d2d_atan2(ma[1] - y0, ma[0] - x0) * D2D_GAZE_RAD2DEG;
}
D2D_GAZE_QUAL double d2d_gaze_agent_pull(const double *mj, double x0, double y0) {
  return d2d_gaze_norm(mj[2], mj[3]) / d2d_gaze_norm(mj[0] - x0, mj[1] - y0);
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_gaze_act / d2d_gaze_reset as plain loops over host arrays (tests/csrc/gaze_host.c), same layouts ---- */

/* Owl.plan of one env.  act, kf: the env's [N] and [N][20]; st: its [D2D_GAZE_OWL_STATE_F].  Returns the action */
D2D_GAZE_QUAL double d2d_gaze_owl_env(const double *dr, const double *tg, const uint8_t *act, const double *kf, int N, double *st,
                                      const double *tab, double w) {
  const double left = st[D2D_GAZE_OWL_S_LEFT];
  if (left > 0.0) { /* `if len(self.u) != 0: return self.u.pop() / top` */
    st[D2D_GAZE_OWL_S_LEFT] = left - 1.0;
    return st[D2D_GAZE_OWL_S_RATE] / w;
  }
  const double x0 = dr[0], y0 = dr[1], yaw = dr[2], vx = dr[3], vy = dr[4];
  const double half = tab[D2D_GAZE_T_FOV] * 0.5, depth = tab[D2D_GAZE_T_DEPTH];
  const double hp = d2d_gaze_mod360(half), hn = d2d_gaze_mod360(-half), ym = d2d_gaze_mod360(-yaw);
  for (int k = 0; k < D2D_GAZE_NDIR; ++k) st[k] = d2d_gaze_score(st[k], k, vx, vy, ym, tab, half, depth);
  const double vn = d2d_gaze_norm(vx, vy);
  const double d_g = d2d_atan2(tg[1] - y0, tg[0] - x0) * D2D_GAZE_RAD2DEG;
  const double d_v = d2d_atan2(vy / vn, vx / vn) * D2D_GAZE_RAD2DEG;
  const double goal_unknown = 1.0 - st[d2d_gaze_nearest(d2d_gaze_mod360(d_g))];
  const double flight_unknown = 1.0 - st[d2d_gaze_nearest(d2d_gaze_mod360(d_v))];
  const double speed2 = d2d_pow2(d2d_gaze_norm(vx / 10.0, vy / 10.0));
  int best = 0;
  double best_c = 0.0;
  for (int i = 0; i < D2D_GAZE_NRATE; ++i) {
    const double h = -(yaw + tab[D2D_GAZE_T_RATE08 + i]);
    const double t0 = d2d_gaze_unseen(h - d_g, half, hp, hn) * goal_unknown;
    const double t1 = (speed2 * d2d_gaze_unseen(h - d_v, half, hp, hn)) * flight_unknown;
    double t2 = 0.0;
    for (int k = 0, j = 0; k < N; ++k) { /* the j-th active tracker's direction with tracker j's state */
      if (!act[k]) continue;
      const double d_o = d2d_gaze_agent_dir(kf + (size_t)k * D2D_GAZE_KF, x0, y0);
      t2 += d2d_gaze_agent_pull(kf + (size_t)j * D2D_GAZE_KF, x0, y0) * d2d_gaze_unseen(h - d_o, half, hp, hn);
      ++j;
    }
    const double cost = d2d_gaze_cost(t0, t1, t2, st[d2d_gaze_nearest(d2d_gaze_mod360(h))], tab[D2D_GAZE_T_TURN + i]);
    if (i == 0 || d2d_gaze_better(cost, best_c)) {
      best = i;
      best_c = cost;
    }
  }
  st[D2D_GAZE_OWL_S_RATE] = tab[D2D_GAZE_T_RATE + best];
  st[D2D_GAZE_OWL_S_LEFT] = tab[D2D_GAZE_T_HOLD];
  return tab[D2D_GAZE_T_ACT + best];
}

/* the argument checks of d2d_gaze_act: 0, -1 or -4 */
D2D_GAZE_QUAL int d2d_gaze_check(const d2d_gaze_call *c) {
  if (!c) return -1;
  if (c->B < 1 || c->N < 0) return -1;
  if (c->N > D2D_GAZE_MAX_N) return -4;
  if (c->kind != D2D_GAZE_K_LOOKAHEAD && c->kind != D2D_GAZE_K_OWL) return -1;
  if (!(c->dt > 0.0) || !(c->yaw_rate_max > 0.0)) return -1;
  if (!c->drone || !c->action) return -1;
  if (c->kind == D2D_GAZE_K_OWL && (!c->target || !c->owl_state || !c->owl_tab || (c->N > 0 && (!c->active || !c->kf)))) return -1;
  return 0;
}

D2D_GAZE_QUAL int d2d_gaze_act_seq(const d2d_gaze_call *c) {
  const int rc = d2d_gaze_check(c);
  if (rc) return rc;
  for (size_t b = 0; b < (size_t)c->B; ++b) {
    if (c->flags && c->flags[b * 4 + D2D_GAZE_F_DONE]) continue;
    const double *dr = c->drone + b * D2D_GAZE_DF;
    if (c->kind == D2D_GAZE_K_LOOKAHEAD)
      c->action[b] = d2d_gaze_lookahead(dr[3], dr[4], dr[2], c->dt, c->yaw_rate_max);
    else
      c->action[b] = d2d_gaze_owl_env(dr, c->target + 2 * b, c->N ? c->active + b * c->N : NULL,
                                      c->N ? c->kf + b * c->N * D2D_GAZE_KF : NULL, c->N, c->owl_state + b * D2D_GAZE_OWL_STATE_F,
                                      c->owl_tab, c->yaw_rate_max);
  }
  return 0;
}

D2D_GAZE_QUAL int d2d_gaze_reset_seq(double *owl_state, const uint8_t *mask, int mask_stride, int B) {
  if (B < 1 || mask_stride < 1 || !owl_state) return -1;
  for (size_t b = 0; b < (size_t)B; ++b) {
    if (mask && !mask[b * mask_stride]) continue;
    for (int f = 0; f < D2D_GAZE_OWL_STATE_F; ++f) owl_state[b * D2D_GAZE_OWL_STATE_F + f] = 0.0;
  }
  return 0;
}
#endif

#endif /* D2D_GAZE_IMPL_H */
