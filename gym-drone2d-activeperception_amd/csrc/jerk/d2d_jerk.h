/*
 * d2d_jerk.h — per-element arithmetic of the Jerk_Primitive planner (include/d2d_jerk.h names the reference lines).
 *
 * The reference (traj_planner.py:403-516) decides, for a drone at p0 with velocity v0, acceleration a0 and goal g:
 *
 *   phi_h     = math.degrees(math.atan2(g.y - p0.y, g.x - p0.x))          d2d_atan2, then one multiplication by 180 / pi
 *   cost(th)  = d ** 2, d = abs(th - phi_h % 360) folded at 180             Python's float %, libm's pow(d, 2.0) (d2d_pow2)
 *   order     = cost.argsort()                                             (cost, index) ranks + the host's tie table
 *   per heading, in that order:
 *     pf = p0 + (delt_x, delt_y); l = g - pf; vf = (0.5 v_max / norm(l)) l; af = 0
 *     delt_a = af - a0; delt_v = vf - v0 - a0 T; delt_p = pf - p0 - v0 T - 0.5 a0 T**2
 *     alpha = delt_a 60 / T**3 - delt_v 360 / T**4 + delt_p 720 / T**5
 *     beta  = -delt_a 24 / T**2 + delt_v 168 / T**3 - delt_p 360 / T**4
 *     gamma = delt_a 3 / T - delt_v 24 / T**2 + delt_p 60 / T**3
 *     p(tt) = alpha / 120 tt**5 + beta / 24 tt**4 + gamma / 6 tt**3 + a0 / 2 tt**2 + v0 tt + p0     (v, a alike)
 *     free iff every sample passes Planner.is_free
 *   the first free heading's (p, v, a) at tt[0]
 *
 * delt_x, delt_y, T and its powers, tt and its powers come from the host's tables (numpy's cos, sin and scalar ** are the host
 * libm's).  Every binary operation is written in Python's order of evaluation (left to right, ** before * and /).
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add.  The scalar pieces are shared by the device kernel (d2d_jerk.hip) and by the plain loop at the end of this file (host
 * builds only), which the CPU tests compare with a Python model bit for bit.
 */
#ifndef D2D_JERK_IMPL_H
#define D2D_JERK_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_jerk.h"

#ifndef D2D_JERK_QUAL
#define D2D_JERK_QUAL static inline
#endif
#ifndef D2D_ATAN2_QUAL
#define D2D_ATAN2_QUAL D2D_JERK_QUAL
#endif
#ifndef D2D_POW2_QUAL
#define D2D_POW2_QUAL D2D_JERK_QUAL
#endif
#include "../d2d_atan2.h"
#include "../d2d_pow2.h"

#define D2D_JERK_OCCUPIED 1  /* grid_type['OCCUPIED'] */
#define D2D_JERK_KF 20       /* doubles of one Kalman record, mu first (D2D_KF of include/d2d.h) */
#define D2D_JERK_DF 8        /* doubles of one drone record: x, y, yaw, vx, vy, ax, ay (D2D_D_* of include/d2d.h) */

/* numpy.linalg.norm of a 2-vector: sqrt(ddot) = sqrt(fma(y, y, x * x)) (d2d_vo_norm of metrics/d2d_vo.h, restated) */
D2D_JERK_QUAL double d2d_jerk_norm(double x, double y) { return __builtin_sqrt(D2D_FMA(y, y, x * x)); }

/* Python's float `a % 360.0` (py_mod360 of d2d_hip.hip, restated): the exact fmod without a loop, then the sign fix-up with one
 * rounded add */
D2D_JERK_QUAL double d2d_jerk_mod360(double a) {
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

/* Python / numpy `int(v // s)` for integer-valued s > 0 (cell_fast of d2d_hip.hip, restated): the exact mathematical floor */
D2D_JERK_QUAL int d2d_jerk_cell(double v, double s, double inv_s) {
  const double q = __builtin_floor(v * inv_s);
  const double r = D2D_FMA(-q, s, v);
  return (int)q + ((r >= s) ? 1 : 0) - ((r < 0.0) ? 1 : 0);
}

/* the same, kept inside [0, hi]: only the address has to be valid where the caller's W_px and W disagree */
D2D_JERK_QUAL int d2d_jerk_cell_in(double v, double s, double inv_s, int hi) {
  const int q = d2d_jerk_cell(v, s, inv_s);
  return q < 0 ? 0 : q > hi ? hi : q;
}

/* byte of cell (i, j) inside one env's grid (grid_ix of d2d_hip.hip, restated) */
D2D_JERK_QUAL size_t d2d_jerk_grid_bytes(int W, int H, int tile) {
  return tile ? (size_t)((W + 15) >> 4) * (size_t)((H + 15) >> 4) * 256 : (size_t)W * (size_t)H;
}
D2D_JERK_QUAL int d2d_jerk_grid_ix(int i, int j, int H, int tile) {
  return tile ? ((((i >> 4) * ((H + 15) >> 4) + (j >> 4)) << 8) | ((i & 15) << 4) | (j & 15)) : i * H + j;
}

/* traj_planner.py:473 */
D2D_JERK_QUAL double d2d_jerk_phi(double px, double py, double gx, double gy) {
  return d2d_atan2(gy - py, gx - px) * 0x1.ca5dc1a63c1f8p+5; /* math.degrees: r * (180 / pi) */
}

/* traj_planner.py:478 for heading index i (theta = 5 i), pm = phi_h % 360 */
D2D_JERK_QUAL double d2d_jerk_cost(int i, double pm) {
  double d = __builtin_fabs((double)(5 * i) - pm);
  if (!(d <= 180.0)) d = 360.0 - d;
  return d2d_pow2(d);
}

/* the weak-order pattern a goal direction falls in: 4 * (bin of 5 degrees) + {0: on the heading, 1: lower half, 2: midway, 3: upper
 * half}.  Only a guess of which row of the tie table to try: the row is used after it has been checked against the costs */
D2D_JERK_QUAL int d2d_jerk_pattern(double pm) {
  if (!(pm >= 0.0 && pm < 360.0)) return 0;
  const int k = (int)__builtin_floor(pm / 5.0);
  const double r = pm - 5.0 * (double)k;
  const int kind = r == 0.0 ? 0 : r < 2.5 ? 1 : r == 2.5 ? 2 : 3;
  return 4 * (k < D2D_JERK_NTHETA ? k : D2D_JERK_NTHETA - 1) + kind;
}

/* the six coefficients of one heading's primitive (alpha, beta, gamma per axis) */
typedef struct d2d_jerk_prim {
  double al[2], be[2], ga[2];
} d2d_jerk_prim;

/* traj_planner.py:417-450.  th: the heading's th_tab row; p0, v0, a0, g: two doubles each */
D2D_JERK_QUAL void d2d_jerk_primitive(const double *th, const double *p0, const double *v0, const double *a0, const double *g,
                                      double half_v_max, d2d_jerk_prim *q) {
  const double T = th[2], T2 = th[3], T3 = th[4], T4 = th[5], T5 = th[6];
  const double pf[2] = {p0[0] + th[0], p0[1] + th[1]};
  const double lx = g[0] - pf[0], ly = g[1] - pf[1];
  const double k = half_v_max / d2d_jerk_norm(lx, ly);
  const double vf[2] = {k * lx, k * ly};
  for (int ii = 0; ii < 2; ++ii) {
    const double da = 0.0 - a0[ii];
    const double dv = vf[ii] - v0[ii] - a0[ii] * T;
    const double dp = pf[ii] - p0[ii] - v0[ii] * T - 0.5 * a0[ii] * T2;
    q->al[ii] = da * 60.0 / T3 - dv * 360.0 / T4 + dp * 720.0 / T5;
    q->be[ii] = -da * 24.0 / T2 + dv * 168.0 / T3 - dp * 360.0 / T4;
    q->ga[ii] = da * 3.0 / T - dv * 24.0 / T2 + dp * 60.0 / T3;
  }
}

/* traj_planner.py:458-460 on axis ii at the sample whose tt_tab row is tt (tt, tt**2 .. tt**5) */
D2D_JERK_QUAL double d2d_jerk_pos(const d2d_jerk_prim *q, int ii, const double *tt, double p0, double v0, double a0) {
  return q->al[ii] / 120.0 * tt[4] + q->be[ii] / 24.0 * tt[3] + q->ga[ii] / 6.0 * tt[2] + a0 / 2.0 * tt[1] + v0 * tt[0] + p0;
}
D2D_JERK_QUAL double d2d_jerk_vel(const d2d_jerk_prim *q, int ii, const double *tt, double v0, double a0) {
  return q->al[ii] / 24.0 * tt[3] + q->be[ii] / 6.0 * tt[2] + q->ga[ii] / 2.0 * tt[1] + a0 * tt[0] + v0;
}
D2D_JERK_QUAL double d2d_jerk_acc(const d2d_jerk_prim *q, int ii, const double *tt, double a0) {
  return q->al[ii] / 6.0 * tt[2] + q->be[ii] / 2.0 * tt[1] + q->ga[ii] * tt[0] + a0;
}

/* the five get_grid probes of Planner.is_free (traj_planner.py:32-52, utils.py:545-548) around (x, y), neither a NaN: 1 if any is
 * OCCUPIED or lies outside the map.  dm: one env's grid.  A probe outside the map reads a clamped cell that is not looked at */
D2D_JERK_QUAL int d2d_jerk_wall(const uint8_t *dm, int W, int H, int tile, double scale, double inv_scale, double W_px, double H_px,
                                double safe, double x, double y) {
  const double xl = x - safe, xr = x + safe, yl = y - safe, yr = y + safe;
  const int ox0 = (xl >= W_px) | (xl < 0.0), ox1 = (x >= W_px) | (x < 0.0), ox2 = (xr >= W_px) | (xr < 0.0);
  const int oy0 = (yl >= H_px) | (yl < 0.0), oy1 = (y >= H_px) | (y < 0.0), oy2 = (yr >= H_px) | (yr < 0.0);
#define D2D_JERK_CLAMPED(v, o, hi) d2d_jerk_cell_in((o) ? 0.0 : (v), scale, inv_scale, (hi))
  const int i0 = D2D_JERK_CLAMPED(xl, ox0, W - 1), i1 = D2D_JERK_CLAMPED(x, ox1, W - 1), i2 = D2D_JERK_CLAMPED(xr, ox2, W - 1);
  const int j0 = D2D_JERK_CLAMPED(yl, oy0, H - 1), j1 = D2D_JERK_CLAMPED(y, oy1, H - 1), j2 = D2D_JERK_CLAMPED(yr, oy2, H - 1);
#undef D2D_JERK_CLAMPED
  const uint8_t v0 = dm[d2d_jerk_grid_ix(i0, j1, H, tile)], v1 = dm[d2d_jerk_grid_ix(i1, j1, H, tile)],
                v2 = dm[d2d_jerk_grid_ix(i2, j1, H, tile)], v3 = dm[d2d_jerk_grid_ix(i1, j0, H, tile)],
                v4 = dm[d2d_jerk_grid_ix(i1, j2, H, tile)];
  return (ox0 | oy1 | (v0 == D2D_JERK_OCCUPIED)) | (ox1 | oy1 | (v1 == D2D_JERK_OCCUPIED)) | (ox2 | oy1 | (v2 == D2D_JERK_OCCUPIED)) |
         (ox1 | oy0 | (v3 == D2D_JERK_OCCUPIED)) | (ox1 | oy2 | (v4 == D2D_JERK_OCCUPIED));
}

/* traj_planner.py:54-58 against the na active trackers staged as five planes trk [5][cap]: mu (x, y, vx, vy), then the limit
 * drone_radius + radius + 5 + var_cam */
D2D_JERK_QUAL int d2d_jerk_hits(const double *trk, int cap, int na, double x, double y, double t) {
  int hit = 0;
  for (int k = 0; k < na; ++k) {
    const double nx = trk[k] + t * trk[2 * cap + k], ny = trk[cap + k] + t * trk[3 * cap + k];
    hit |= d2d_jerk_norm(x - nx, y - ny) <= trk[4 * cap + k];
  }
  return hit;
}

/* what the planner reads of one env, and where a sample of heading `th` is free */
typedef struct d2d_jerk_env {
  double p0[2], v0[2], a0[2], g[2];
  const uint8_t *dm;
  const double *trk;
  int cap, na;
  double inv_scale, safe;
} d2d_jerk_env;

/* is sample s of the primitive q of heading index th free? (Planner.is_free) */
D2D_JERK_QUAL int d2d_jerk_sample_free(const d2d_jerk_call *c, const d2d_jerk_env *e, const d2d_jerk_prim *q, int th, int s) {
  const double *tt = c->tt_tab + ((size_t)th * c->S + s) * D2D_JERK_TT_F;
  const double x = d2d_jerk_pos(q, 0, tt, e->p0[0], e->v0[0], e->a0[0]), y = d2d_jerk_pos(q, 1, tt, e->p0[1], e->v0[1], e->a0[1]);
  if (x != x || y != y) return 0;
  if (d2d_jerk_wall(e->dm, c->W, c->H, c->grid_tile, c->scale, e->inv_scale, c->W_px, c->H_px, e->safe, x, y)) return 0;
  return !d2d_jerk_hits(e->trk, e->cap, e->na, x, y, tt[0]);
}

/* the heading's `times`, kept inside [1, S] whatever the table holds */
D2D_JERK_QUAL int d2d_jerk_times(const d2d_jerk_call *c, int th) {
  const double t = c->th_tab[(size_t)th * D2D_JERK_TH_F + 7];
  return t >= 1.0 ? (t <= (double)c->S ? (int)t : c->S) : 1;
}

/* Does row `pat` of the tie table describe the weak order of cost[72]?  seen: 72 bytes of scratch */
D2D_JERK_QUAL int d2d_jerk_table_fits(const d2d_jerk_call *c, int pat, const double *cost, uint8_t *seen) {
  const uint8_t *perm = c->tie_perm + (size_t)pat * D2D_JERK_NTHETA, *eq = c->tie_eq + (size_t)pat * D2D_JERK_NTHETA;
  for (int r = 0; r < D2D_JERK_NTHETA; ++r) seen[r] = 0;
  for (int r = 0; r < D2D_JERK_NTHETA; ++r) {
    if (perm[r] >= D2D_JERK_NTHETA || seen[perm[r]]) return 0;
    seen[perm[r]] = 1;
  }
  for (int r = 0; r + 1 < D2D_JERK_NTHETA; ++r) {
    const double a = cost[perm[r]], b = cost[perm[r + 1]];
    if (!(eq[r] ? a == b : a < b)) return 0;
  }
  return 1;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_jerk_plan as a plain loop over host arrays (tests/csrc/jerk_host.c), same layouts as include/d2d_jerk.h ---- */

/* `work`: 5 * max(N, 1) doubles of scratch (the active trackers of one env); returns 0, or -4 above the limits */
D2D_JERK_QUAL int d2d_jerk_plan_seq(const d2d_jerk_call *c, double *work) {
  const int N = c->N, cap = N > 0 ? N : 1;
  if (N > D2D_JERK_MAX_N || c->S > D2D_JERK_MAX_S || c->S < 1) return -4;
  const size_t gb = d2d_jerk_grid_bytes(c->W, c->H, c->grid_tile);
  for (int b = 0; b < c->B; ++b) {
    const double *dr = c->drone + (size_t)b * D2D_JERK_DF;
    d2d_jerk_env e = {{dr[0], dr[1]}, {dr[3], dr[4]}, {dr[5], dr[6]}, {c->target[2 * (size_t)b], c->target[2 * (size_t)b + 1]},
                      c->dmap + (size_t)b * gb, work, cap, 0, 1.0 / c->scale, c->drone_radius + 10.0};
    for (int k = 0; k < N; ++k) { /* utils.py:184, 238 and the active trackers */
      const size_t ik = (size_t)b * N + k;
      const int act = c->active[ik] != 0;
      if (c->trk_prev[ik] && !act) c->trk_radius[ik] = c->agent_radius;
      c->trk_prev[ik] = (uint8_t)act;
      if (!act) continue;
      const double *mu = c->kf + ik * D2D_JERK_KF;
      for (int f = 0; f < 4; ++f) work[f * cap + e.na] = mu[f];
      work[4 * cap + e.na] = c->drone_radius + c->trk_radius[ik] + 5.0 + c->var_cam;
      ++e.na;
    }
    const double pm = d2d_jerk_mod360(d2d_jerk_phi(e.p0[0], e.p0[1], e.g[0], e.g[1]));
    double cost[D2D_JERK_NTHETA];
    int order[D2D_JERK_NTHETA], tie = 0;
    uint8_t seen[D2D_JERK_NTHETA];
    for (int i = 0; i < D2D_JERK_NTHETA; ++i) cost[i] = d2d_jerk_cost(i, pm), order[i] = i;
    if (pm == pm)
      for (int i = 0; i < D2D_JERK_NTHETA; ++i) {
        int r = 0;
        for (int j = 0; j < D2D_JERK_NTHETA; ++j) r += cost[j] < cost[i] || (cost[j] == cost[i] && j < i);
        order[r] = i;
      }
    for (int r = 0; r + 1 < D2D_JERK_NTHETA; ++r) tie |= cost[order[r]] == cost[order[r + 1]];
    const int pat = d2d_jerk_pattern(pm);
    int stat = 0;
    if (d2d_jerk_table_fits(c, pat, cost, seen))
      for (int r = 0; r < D2D_JERK_NTHETA; ++r) order[r] = c->tie_perm[(size_t)pat * D2D_JERK_NTHETA + r];
    else if (tie || pm != pm)
      stat |= D2D_JERK_STAT_UNKNOWN;
    int found = -1, tested = 0;
    d2d_jerk_prim q;
    for (int r = 0; r < D2D_JERK_NTHETA && found < 0; ++r) {
      const int th = order[r], times = d2d_jerk_times(c, th);
      int fr = 1;
      d2d_jerk_primitive(c->th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c->half_v_max, &q);
      for (int s = 0; s < times && fr; ++s) fr = d2d_jerk_sample_free(c, &e, &q, th, s);
      ++tested;
      if (fr) found = r;
    }
    double *wp = c->wp + (size_t)b * 6;
    if (found >= 0) {
      const int th = order[found];
      const double *tt = c->tt_tab + (size_t)th * c->S * D2D_JERK_TT_F;
      for (int ii = 0; ii < 2; ++ii) {
        wp[ii] = d2d_jerk_pos(&q, ii, tt, e.p0[ii], e.v0[ii], e.a0[ii]);
        wp[2 + ii] = d2d_jerk_vel(&q, ii, tt, e.v0[ii], e.a0[ii]);
        wp[4 + ii] = d2d_jerk_acc(&q, ii, tt, e.a0[ii]);
      }
      if (found + 1 < D2D_JERK_NTHETA && cost[order[found + 1]] == cost[th]) { /* would the tied neighbour have been taken too? */
        const int t2 = order[found + 1], times = d2d_jerk_times(c, t2);
        int fr = 1;
        d2d_jerk_primitive(c->th_tab + (size_t)t2 * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c->half_v_max, &q);
        for (int s = 0; s < times && fr; ++s) fr = d2d_jerk_sample_free(c, &e, &q, t2, s);
        if (fr) stat |= D2D_JERK_STAT_TIE;
      }
      c->choice[b] = th;
    } else {
      for (int i = 0; i < 6; ++i) wp[i] = 0.0;
      c->choice[b] = -1;
    }
    c->plan_ok[b] = c->wp_valid[b] = (uint8_t)(found >= 0);
    c->stat[b] = stat | (tested << D2D_JERK_STAT_SHIFT);
  }
  return 0;
}

D2D_JERK_QUAL void d2d_jerk_reset_seq(double *trk_radius, uint8_t *trk_prev, const double *trk_radius0, const uint8_t *mask,
                                      int mask_stride, int B, int N) {
  for (int b = 0; b < B; ++b) {
    if (mask && !mask[(size_t)b * mask_stride]) continue;
    for (int k = 0; k < N; ++k) trk_radius[(size_t)b * N + k] = trk_radius0[(size_t)b * N + k], trk_prev[(size_t)b * N + k] = 0;
  }
}
#endif

#endif /* D2D_JERK_IMPL_H */
