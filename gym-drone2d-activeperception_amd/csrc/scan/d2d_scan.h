/*
 * d2d_scan.h — per-sample arithmetic of the per-ray scan (include/d2d_scan.h names the reference lines).
 *
 * Raycast.castRay (utils.py:620-713) for one ray as IEEE-754 binary64 operations in the reference's own order:
 *   math.radians(yaw)          yaw * (pi / 180), one multiplication
 *   get_positive_angle         copysign(fmod(|a|, 2 pi), a), + 2 pi where negative (:612-618)
 *   tan                        d2d_tan (../d2d_tan.h), the host libm's bits
 *   a ** 2                     a * a
 *   int(x // scale)            the floor of the exact quotient (d2d_scan_cell)
 *   x = x + x_step             the iterated sums themselves: what `coords` holds
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one operation, every D2D_FMA one fused multiply-add.  The ray
 * (d2d_scan_ray) and its per-sample body (d2d_scan_sample) are shared by the device kernel (d2d_scan.hip) and by the plain loop at the
 * end of this file (host builds only), which the CPU tests compare with the Python model ray for ray.
 */
#ifndef D2D_SCAN_IMPL_H
#define D2D_SCAN_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_scan.h"

#ifndef D2D_SCAN_QUAL
#define D2D_SCAN_QUAL static inline
#endif
#ifndef D2D_TAN_QUAL
#define D2D_TAN_QUAL D2D_SCAN_QUAL
#endif
#ifndef D2D_SCAN_CHECK_QUAL
#define D2D_SCAN_CHECK_QUAL static inline /* the argument checks run on the host in every build */
#endif
#include "../d2d_tan.h"

#define D2D_SCAN_DEG2RAD 0x1.1df46a2529d39p-6 /* pi / 180 */
#define D2D_SCAN_TWO_PI 0x1.921fb54442d18p+2  /* math.pi * 2 */
#define D2D_SCAN_CCAP 64                      /* candidates of one env the culled list holds; an env with more tests every agent */

/* the agents a ray's samples can meet and the grid they read: one env's view of the world */
typedef struct d2d_scan_view {
  const double *cx, *cy, *cr2; /* [ncand] centre and radius ** 2 of every candidate */
  const int32_t *cidx;         /* [ncand] the candidate's agent, NULL: candidate q is agent q */
  int32_t ncand;
  int32_t W, H, tile;          /* the grid of `gt` (d2d_cfg.W, H, grid_tile) */
  const uint8_t *gt;           /* this env's ground truth */
  double scale, W_px, H_px, depth2, x0, y0;
  int32_t max_samples;         /* a bound no ray reaches: the longer side over the step, and a few */
} d2d_scan_view;

/* fmod(a, b) for a >= 0, b > 0 with 1 / b at hand: the remainder is exact in one fused operation */
D2D_SCAN_QUAL double d2d_scan_fmod_pos(double a, double b, double inv_b) {
  const double n = __builtin_trunc(a * inv_b);
  double m = D2D_FMA(-n, b, a);
  if (m < 0.0) m = D2D_FMA(-(n - 1.0), b, a);
  else if (m >= b) m = D2D_FMA(-(n + 1.0), b, a);
  return m;
}

/* utils.py:612-618 */
D2D_SCAN_QUAL double d2d_scan_positive_angle(double a) {
  a = __builtin_copysign(d2d_scan_fmod_pos(__builtin_fabs(a), D2D_SCAN_TWO_PI, 0x1.45f306dc9c883p-3 /* 1 / (2 pi) */), a);
  if (a < 0.0) a += D2D_SCAN_TWO_PI;
  return a;
}

/* the steps of ray i of a drone with yaw `yaw` degrees (utils.py:594, :621-650, :682-683); ss = scale - 1 */
D2D_SCAN_QUAL void d2d_scan_steps(double yaw, double ray_off0, double ray_dth, int i, double ss, double *xs, double *ys) {
  const double rad90 = 0x1.921fb54442d18p+0, rad270 = 0x1.2d97c7f3321d2p+2, pi_ = 0x1.921fb54442d18p+1;
  const double player_angle = D2D_SCAN_TWO_PI - yaw * D2D_SCAN_DEG2RAD;
  const double ang = d2d_scan_positive_angle(player_angle + (ray_off0 + ray_dth * (double)i));
  const int faced_right = (ang < rad90 || ang > rad270), faced_up = (ang > pi_);
  double slope = d2d_tan(ang);
  if (__builtin_fabs(slope) > 1.0) {
    slope = 1.0 / slope;
    *ys = faced_up ? -ss : ss;
    *xs = *ys * slope;
  } else {
    *xs = faced_right ? ss : -ss;
    *ys = *xs * slope;
  }
}

/* int(v // s) for 0 < v, s > 0, clamped to [0, n - 1]: the index of a cell of the grid whatever v holds */
D2D_SCAN_QUAL int d2d_scan_cell(double v, double s, int n) {
  double q = __builtin_floor(v / s);
  const double r = D2D_FMA(-q, s, v); /* the quotient's rounding may have crossed an integer: at most one correction applies */
  if (r >= s) q += 1.0;
  if (r < 0.0) q -= 1.0;
  if (!(q >= 0.0)) return 0;
  if (q > (double)(n - 1)) return n - 1;
  return (int)q;
}

/* byte of cell (i, j) inside one env's grid (d2d_cfg.grid_tile): 0 <= i < W, 0 <= j < H */
D2D_SCAN_QUAL size_t d2d_scan_grid_ix(int i, int j, int H, int tile) {
  return tile ? (((size_t)(i >> 4) * (size_t)((H + 15) >> 4) + (size_t)(j >> 4)) << 8) | (size_t)(((i & 15) << 4) | (j & 15))
              : (size_t)i * (size_t)H + (size_t)j;
}

D2D_SCAN_QUAL int d2d_scan_inside(const d2d_scan_view *v, double x, double y) {
  return 0.0 < x && x < v->W_px && 0.0 < y && y < v->H_px;
}

/* can an agent with radius ** 2 = r2 at (px, py) hold a sample of this drone's rays?  A sample that is tested is the drone's own
 * position or follows one nearer than depth, a step being at most sqrt(2) * ss long: it lies within depth + sqrt(2) * ss of the
 * drone.  A bound only; the exact test of d2d_scan_sample decides.  (NaN anywhere: no, and no sample passes the exact test either) */
D2D_SCAN_QUAL int d2d_scan_near(double px, double py, double r2, double x0, double y0, double depth, double ss) {
  const double lim = __builtin_sqrt(r2) + depth + 1.5 * ss + 2.0;
  const double dx = px - x0, dy = py - y0;
  return dx * dx + dy * dy <= lim * lim;
}

/* one sample inside the map (utils.py:655-674): 0 = the ray goes on, else the kind of its stop.  `hit`: the ray's own words */
D2D_SCAN_QUAL int d2d_scan_sample(const d2d_scan_view *v, double x, double y, uint32_t *hit) {
  int any = 0;
  for (int q = 0; q < v->ncand; ++q) { /* every agent, no early-out among them (:658-662) */
    const double dx = v->cx[q] - x, dy = v->cy[q] - y;
    if (dx * dx + dy * dy <= v->cr2[q]) {
      const int k = v->cidx ? v->cidx[q] : q;
      hit[k >> 5] |= 1u << (k & 31);
      any = 1;
    }
  }
  if (any) return 2;
  const int i = d2d_scan_cell(x, v->scale, v->W), j = d2d_scan_cell(y, v->scale, v->H);
  const uint8_t wall = v->gt[d2d_scan_grid_ix(i, j, v->H, v->tile)];
  const double dist = (x - v->x0) * (x - v->x0) + (y - v->y0) * (y - v->y0);
  if (wall == D2D_OCCUPIED) return 1;
  if (dist >= v->depth2) return 3;
  return 0;
}

/* castRay with the steps (xs, ys): the ray's record.  A ray of a drone outside the map takes no sample and reads no cell */
D2D_SCAN_QUAL void d2d_scan_ray(const d2d_scan_view *v, double xs, double ys, int hit_words, double *end, uint8_t *kind, uint32_t *hit,
                                float *range, float *outcome) {
  for (int w = 0; w < hit_words; ++w) hit[w] = 0u;
  double x = v->x0, y = v->y0, lx = x, ly = y;
  int k = 0, taken = 0;
  for (int n = 0; n < v->max_samples && d2d_scan_inside(v, x, y); ++n) {
    lx = x;
    ly = y;
    taken = 1;
    k = d2d_scan_sample(v, x, y, hit);
    if (k) break;
    x = x + xs;
    y = y + ys;
  }
  end[0] = k ? lx : -1.0;
  end[1] = k ? ly : -1.0;
  *kind = (uint8_t)k;
  const double dx = lx - v->x0, dy = ly - v->y0;
  *range = taken ? (float)__builtin_sqrt(dx * dx + dy * dy) : 0.0f;
  *outcome = (float)k;
}

/* is there anything to do for an env whose counter says `steps` and whose latest update was at `last`? */
D2D_SCAN_QUAL int d2d_scan_due(int steps, int last) { return steps >= 1 && steps != last; }

D2D_SCAN_QUAL int d2d_scan_max_samples(double W_px, double H_px, double ss) {
  const double n = (W_px > H_px ? W_px : H_px) / ss + 4.0;
  return n < 16777216.0 ? (int)n : 16777216;
}

/* the argument checks of d2d_scan_update: 0 or the error, `*why` the text */
D2D_SCAN_CHECK_QUAL int d2d_scan_check(const d2d_cfg *c, const d2d_state *s, const d2d_scan *w, const char **why) {
  *why = "";
  if (!c || !s || !w) return (*why = "d2d_scan_update: cfg, state or scan is NULL"), -1;
  if (c->abi_version != D2D_ABI_VERSION) return (*why = "d2d_scan_update: the cfg has another D2D_ABI_VERSION"), -2;
  if (!s->agents || !s->gt || !s->counters) return (*why = "d2d_scan_update: agents, gt or counters is NULL"), -1;
  if (!w->pose || !w->end || !w->kind || !w->hit || !w->obs || !w->last_step) return (*why = "d2d_scan_update: a scan buffer is NULL"), -1;
  if (c->B < 0 || c->N < 0 || c->W < 1 || c->H < 1 || c->R < 1 || !(c->scale > 1.0) || !(c->depth >= 0.0) || !(c->W_px > 0.0) ||
      !(c->H_px > 0.0) || !(c->W_px <= 1e9) || !(c->H_px <= 1e9))
    return (*why = "d2d_scan_update: B, N >= 0, W, H, R >= 1, scale > 1, depth >= 0, 0 < W_px, H_px <= 1e9"), -1;
  if (c->grid_tile != 0 && c->grid_tile != 16) return (*why = "d2d_scan_update: grid_tile is 0 or 16"), -1;
  if (c->N > 0x7fffffff - 31 || D2D_GRID_BYTES(c) > (size_t)0x7fffffff)
    return (*why = "d2d_scan_update: N and the bytes of a grid are 32-bit indices"), -4;
  if (w->hit_words < 1 || w->hit_words < (c->N + 31) / 32) return (*why = "d2d_scan_update: hit_words >= max(1, ceil(N / 32))"), -1;
  if ((long long)c->R * w->hit_words > 0x7fffffffll) return (*why = "d2d_scan_update: R * hit_words is a 32-bit index"), -4;
  return 0;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_scan_update as a plain loop over host arrays (tests/csrc/scan_host.c), same layouts ---- */
D2D_SCAN_QUAL int d2d_scan_update_seq(const d2d_cfg *c, const d2d_state *s, const d2d_scan *w) {
  const char *why;
  const int rc = d2d_scan_check(c, s, w, &why);
  if (rc) return rc;
  const int N = c->N, R = c->R, hw = w->hit_words;
  const double ss = c->scale - 1.0;
  const size_t gb = D2D_GRID_BYTES(c);
  for (size_t e = 0; e < (size_t)c->B; ++e) {
    const int steps = s->counters[e * D2D_CF + D2D_C_STEPS];
    if (!d2d_scan_due(steps, w->last_step[e])) continue;
    const double *pose = w->pose + e * D2D_DF, *ag = s->agents + e * D2D_AF * (size_t)N;
    const double *ax = ag + (size_t)D2D_A_PX * N, *ay = ag + (size_t)D2D_A_PY * N, *ar2 = ag + (size_t)D2D_A_R2 * N;
    double cx[D2D_SCAN_CCAP], cy[D2D_SCAN_CCAP], cr2[D2D_SCAN_CCAP];
    int32_t cidx[D2D_SCAN_CCAP];
    int ncand = 0;
    for (int k = 0; k < N; ++k)
      if (d2d_scan_near(ax[k], ay[k], ar2[k], pose[D2D_D_X], pose[D2D_D_Y], c->depth, ss)) {
        if (ncand < D2D_SCAN_CCAP) cx[ncand] = ax[k], cy[ncand] = ay[k], cr2[ncand] = ar2[k], cidx[ncand] = k;
        ++ncand;
      }
    d2d_scan_view v = {cx, cy, cr2, cidx, ncand, c->W, c->H, c->grid_tile, s->gt + e * gb, c->scale, c->W_px, c->H_px,
                       c->depth * c->depth, pose[D2D_D_X], pose[D2D_D_Y], d2d_scan_max_samples(c->W_px, c->H_px, ss)};
    if (ncand > D2D_SCAN_CCAP) v.cx = ax, v.cy = ay, v.cr2 = ar2, v.cidx = NULL, v.ncand = N;
    for (int i = 0; i < R; ++i) {
      double xs, ys;
      d2d_scan_steps(pose[D2D_D_YAW], c->ray_off0, c->ray_dth, i, ss, &xs, &ys);
      const size_t ray = e * (size_t)R + (size_t)i;
      d2d_scan_ray(&v, xs, ys, hw, w->end + ray * 2, w->kind + ray, w->hit + ray * (size_t)hw, w->obs + e * 2 * (size_t)R + i,
                   w->obs + e * 2 * (size_t)R + R + i);
    }
    w->last_step[e] = steps;
  }
  return 0;
}
#endif

#endif /* D2D_SCAN_IMPL_H */
