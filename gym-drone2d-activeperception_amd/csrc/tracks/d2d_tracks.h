/*
 * d2d_tracks.h — per-element arithmetic of the tracker-forecast map (include/d2d_tracks.h names the reference lines).
 *
 * As IEEE-754 binary64 operations in the reference's own order:
 *   k * dt                              the product of the converted integer and dt (traj_planner.py:224, :227)
 *   estimate_pos(t)                     mu[0] + t * mu[2], mu[1] + t * mu[3]: a multiplication, then an addition (utils.py:223)
 *   get_real_pos(i, j)                  scale * (i + 0.5): i + 0.5 is exact, one multiplication (utils.py:543)
 *   norm(p - e) <= thr                  fma(dy, dy, dx * dx) <= sq_threshold(thr), the plan stage's and k_swept_mark's test
 *                                       (csrc/d2d_plugins.h), restated here as csrc/jerk/d2d_jerk.h restates its pieces
 *   drone_radius + radius + margin      two additions, left to right
 *   int(x // scale)                     the floor of the exact quotient (d2d_tracks_cell)
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one operation, every D2D_FMA one fused multiply-add.  The scalar
 * pieces are shared by the device kernel (d2d_tracks.hip) and by the plain loop at the end of this file (host builds only), which the
 * CPU tests compare with the numpy model cell for cell.
 */
#ifndef D2D_TRACKS_IMPL_H
#define D2D_TRACKS_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_tracks.h"

#ifndef D2D_TRACKS_QUAL
#define D2D_TRACKS_QUAL static inline
#endif
#ifndef D2D_TRACKS_CHECK_QUAL
#define D2D_TRACKS_CHECK_QUAL static inline /* the argument checks run on the host in every build */
#endif
#ifndef D2D_FMA
#define D2D_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

#define D2D_TRACKS_NONE 256u               /* a cell no forecast reaches, in the 32-bit plane the minimum is taken on */
#define D2D_TRACKS_LDS_BYTES 65536          /* what one workgroup may hold without asking for more */

/* The largest double s with sqrt(s) <= r (sqrt correctly rounded, hence monotone): norm(d) <= r with numpy's
 * norm = sqrt(fma(dy, dy, dx * dx)) is exactly fma(dy, dy, dx * dx) <= s.  r * r is within a few ulp of it; the walk is bounded.
 * Nothing is <= a negative or NaN limit: -1 */
D2D_TRACKS_QUAL double d2d_tracks_sq_threshold(double r) {
  if (!(r >= 0.0)) return -1.0;
  double t = r * r;
  long long b;
  for (int k = 0; k < 8 && __builtin_sqrt(t) > r; ++k) {
    __builtin_memcpy(&b, &t, sizeof b);
    b -= 1;
    __builtin_memcpy(&t, &b, sizeof b);
  }
  for (int k = 0; k < 8; ++k) {
    double u;
    __builtin_memcpy(&b, &t, sizeof b);
    b += 1;
    __builtin_memcpy(&u, &b, sizeof b);
    if (!(__builtin_sqrt(u) <= r)) break;
    t = u;
  }
  return t;
}

/* int(v // s) for s > 0, clamped to [-2, limit + 1] so that it fits an int whatever v holds (NaN: -2) */
D2D_TRACKS_QUAL int d2d_tracks_cell(double v, double s, int limit) {
  double q = __builtin_floor(v / s);
  const double r = D2D_FMA(-q, s, v); /* the quotient's rounding may have crossed an integer: at most one correction applies */
  if (r >= s) q += 1.0;
  if (r < 0.0) q -= 1.0;
  if (!(q >= -2.0)) return -2;
  if (q > (double)limit + 1.0) return limit + 1;
  return (int)q;
}

/* the cells [lo, hi] of one axis whose centre can lie within `r` of the coordinate v, one cell of slack on either side, cut to the
 * cells of the window that are inside the map: [max(w0, 0), min(w0 + L, n) - 1].  Empty (lo > hi) for a NaN or a far-away v */
D2D_TRACKS_QUAL void d2d_tracks_span(double v, double r, double s, int n, int w0, int L, int *lo, int *hi) {
  const int a = d2d_tracks_cell(v - r, s, n) - 1, b = d2d_tracks_cell(v + r, s, n) + 1;
  const int first = w0 > 0 ? w0 : 0, last = (w0 + L < n ? w0 + L : n) - 1;
  *lo = a < first ? first : a;
  *hi = b > last ? last : b;
}

/* get_real_pos along one axis: the centre of cell i */
D2D_TRACKS_QUAL double d2d_tracks_centre(int i, double s) { return s * ((double)i + 0.5); }

/* estimate_pos(t) along one axis */
D2D_TRACKS_QUAL double d2d_tracks_estimate(double m, double v, double t) { return m + t * v; }

/* norm((px, py) - (ex, ey)) <= thr, lim = sq_threshold(thr) */
D2D_TRACKS_QUAL int d2d_tracks_hit(double px, double py, double ex, double ey, double lim) {
  const double dx = px - ex, dy = py - ey;
  return D2D_FMA(dy, dy, dx * dx) <= lim;
}

/* is there anything to do for an env whose counter says `steps` and whose latest update was at `last`? */
D2D_TRACKS_QUAL int d2d_tracks_due(int steps, int last, int force) { return force != 0 || steps != last; }

/* LDS of one wave: six planes of the active trackers (mu, velocity, threshold and its squared form), then the 32-bit window plane */
D2D_TRACKS_CHECK_QUAL size_t d2d_tracks_wave_bytes(int N, int L) {
  const size_t trk = ((size_t)(N > 0 ? N : 1) * 6 * sizeof(double) + 15) & ~(size_t)15;
  return trk + (((size_t)L * L * sizeof(uint32_t) + 15) & ~(size_t)15);
}

/* the argument checks of d2d_tracks_update: 0 or the error, `*why` the text */
D2D_TRACKS_CHECK_QUAL int d2d_tracks_check(const d2d_cfg *c, const d2d_state *s, const d2d_tracks *w, const char **why) {
  *why = "";
  if (!c || !s || !w) return (*why = "d2d_tracks_update: cfg, state or tracks is NULL"), -1;
  if (c->abi_version != D2D_ABI_VERSION) return (*why = "d2d_tracks_update: the cfg has another D2D_ABI_VERSION"), -2;
  if (!s->drone || !s->counters) return (*why = "d2d_tracks_update: drone or counters is NULL"), -1;
  if (!w->win || !w->cells || !w->last_step) return (*why = "d2d_tracks_update: a tracks buffer is NULL"), -1;
  if (c->B < 0 || c->N < 0 || c->W < 1 || c->H < 1 || c->L < 1 || !(c->scale > 0.0))
    return (*why = "d2d_tracks_update: B >= 0, N >= 0, W, H, L >= 1, scale > 0"), -1;
  if (c->N > 0 && (!s->kf || !s->active || !w->trk_radius))
    return (*why = "d2d_tracks_update: kf, active or trk_radius is NULL with N > 0"), -1;
  if (w->samples < 1 || w->samples > D2D_TRACKS_MAX_SAMPLES) return (*why = "d2d_tracks_update: samples is 1 .. 255"), -1;
  if ((long long)c->L * c->L > 0x7fffffffll) return (*why = "d2d_tracks_update: L * L is a 32-bit cell index"), -4;
  if (d2d_tracks_wave_bytes(c->N, c->L) > D2D_TRACKS_LDS_BYTES)
    return (*why = "d2d_tracks_update: the trackers and the window of one env do not fit 64 KiB of LDS"), -4;
  return 0;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_tracks_update as a plain loop over host arrays (tests/csrc/tracks_host.c), same layouts.  `plane` is the caller's
 * scratch of L * L uint32 ---- */
D2D_TRACKS_QUAL int d2d_tracks_update_seq(const d2d_cfg *c, const d2d_state *s, const d2d_tracks *w, uint32_t *plane) {
  const char *why;
  const int rc = d2d_tracks_check(c, s, w, &why);
  if (rc) return rc;
  if (!plane) return -1;
  const int N = c->N, W = c->W, H = c->H, L = c->L, edge = (L - 1) / 2, nn = L * L;
  for (size_t e = 0; e < (size_t)c->B; ++e) {
    const int steps = s->counters[e * D2D_CF + D2D_C_STEPS];
    if (!d2d_tracks_due(steps, w->last_step[e], w->force)) continue;
    const double *dr = s->drone + e * D2D_DF;
    const int i0 = d2d_tracks_cell(dr[D2D_D_X], c->scale, W) - edge, j0 = d2d_tracks_cell(dr[D2D_D_Y], c->scale, H) - edge;
    for (int a = 0; a < nn; ++a) plane[a] = D2D_TRACKS_NONE;
    for (int q = 0; q < N; ++q) {
      if (!s->active[e * N + q]) continue;
      const double *mu = s->kf + (e * N + q) * D2D_KF;
      const double thr = c->drone_radius + w->trk_radius[e * N + q] + w->margin, lim = d2d_tracks_sq_threshold(thr);
      if (!(lim >= 0.0)) continue;
      for (int k = 0; k < w->samples; ++k) {
        const double t = (double)k * c->dt;
        const double ex = d2d_tracks_estimate(mu[0], mu[2], t), ey = d2d_tracks_estimate(mu[1], mu[3], t);
        int i_lo, i_hi, j_lo, j_hi;
        d2d_tracks_span(ex, thr, c->scale, W, i0, L, &i_lo, &i_hi);
        d2d_tracks_span(ey, thr, c->scale, H, j0, L, &j_lo, &j_hi);
        for (int i = i_lo; i <= i_hi; ++i)
          for (int j = j_lo; j <= j_hi; ++j)
            if (d2d_tracks_hit(d2d_tracks_centre(i, c->scale), d2d_tracks_centre(j, c->scale), ex, ey, lim)) {
              uint32_t *p = plane + (i - i0) * L + (j - j0);
              if ((uint32_t)(k + 1) < *p) *p = (uint32_t)(k + 1);
            }
      }
    }
    uint8_t *out = w->win + e * (size_t)nn;
    int cells = 0;
    for (int a = 0; a < nn; ++a) {
      const uint32_t v = plane[a];
      out[a] = (uint8_t)(v < D2D_TRACKS_NONE ? v : 0u);
      cells += v < D2D_TRACKS_NONE;
    }
    w->cells[e] = cells;
    w->last_step[e] = steps;
  }
  return 0;
}
#endif

#endif /* D2D_TRACKS_IMPL_H */
