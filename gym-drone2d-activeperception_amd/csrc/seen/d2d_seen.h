/*
 * d2d_seen.h — per-element arithmetic of the time-since-observed map (include/d2d_seen.h names the reference lines).
 *
 * Oxford.get_view_map (yaw_planner.py:67-79) for one cell and the bookkeeping of `last_time_observed_map` (:92-97) as IEEE-754
 * binary64 operations in the reference's own order:
 *   math.radians(d)            d * (pi / 180), one multiplication
 *   math.cos / math.sin        d2d_cos / d2d_sin (../d2d_sincos.h), the host libm's bits
 *   a ** 2 on a numpy array    a * a
 *   np.arccos(q) <= half       the host's 64-double decision window (device_plugins.acos_window); |q| > 1 or NaN: not seen
 *   int(x // scale)            the floor of the exact quotient (d2d_seen_cell)
 *   np.float32(v)              the conversion of the float64 table value, rounded to nearest even
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one operation, every D2D_FMA one fused multiply-add.  The scalar
 * pieces are shared by the device kernel (d2d_seen.hip) and by the plain loop at the end of this file (host builds only), which the
 * CPU tests compare with the numpy model cell for cell.
 */
#ifndef D2D_SEEN_IMPL_H
#define D2D_SEEN_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_seen.h"

#ifndef D2D_SEEN_QUAL
#define D2D_SEEN_QUAL static inline
#endif
#ifndef D2D_SINCOS_QUAL
#define D2D_SINCOS_QUAL D2D_SEEN_QUAL
#endif
#ifndef D2D_SEEN_CHECK_QUAL
#define D2D_SEEN_CHECK_QUAL static inline /* the argument checks run on the host in every build */
#endif
#include "../d2d_sincos.h"

#define D2D_SEEN_DEG2RAD 0x1.1df46a2529d39p-6 /* pi / 180 */

/* monotone integer image of a double: the order of the keys is the order of the doubles (device_plugins._key) */
D2D_SEEN_QUAL long long d2d_seen_key(double x) {
  long long b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}

/* np.arccos(q) <= view_angle (yaw_planner.py:78) through the host's decision window */
D2D_SEEN_QUAL int d2d_seen_acos_le(long long key_lo, unsigned long long mask, double q) {
  if (!(__builtin_fabs(q) <= 1.0)) return 0;
  const long long k = d2d_seen_key(q);
  if (k >= key_lo + 64) return 1;
  if (k < key_lo) return 0;
  return (int)((mask >> (int)(k - key_lo)) & 1ull);
}

/* the view direction of a drone with yaw `yaw` degrees: cos(radians(yaw)), -sin(radians(yaw)) (:72) */
D2D_SEEN_QUAL void d2d_seen_dir(double yaw, double *cy, double *sy) {
  const double r = yaw * D2D_SEEN_DEG2RAD;
  *cy = d2d_cos(r);
  *sy = -d2d_sin(r);
}

/* get_view_map for the cell whose origin is (x, y), seen from (x0, y0) along (cy, sy); depth2 = depth ** 2 */
D2D_SEEN_QUAL int d2d_seen_view(long long key_lo, unsigned long long mask, double depth2, double x0, double y0, double cy, double sy,
                                double x, double y) {
  const double a = x0 - x, b = y0 - y;
  const double d2 = a * a + b * b;
  if (d2 <= 0.0) return 1;
  if (!(d2 <= depth2)) return 0;
  const double dot = (x - x0) * cy + (y - y0) * sy;
  return d2d_seen_acos_le(key_lo, mask, dot / __builtin_sqrt(d2));
}

/* int(v // s) for s > 0, clamped to [-2, limit + 1] so that it fits an int whatever v holds (NaN: -2) */
D2D_SEEN_QUAL int d2d_seen_cell(double v, double s, int limit) {
  double q = __builtin_floor(v / s);
  const double r = D2D_FMA(-q, s, v); /* the quotient's rounding may have crossed an integer: at most one correction applies */
  if (r >= s) q += 1.0;
  if (r < 0.0) q -= 1.0;
  if (!(q >= -2.0)) return -2;
  if (q > (double)limit + 1.0) return limit + 1;
  return (int)q;
}

/* the cells [lo, hi] of one axis (n cells) whose origin can lie within `depth` of the coordinate v: one cell of slack on either side */
D2D_SEEN_QUAL void d2d_seen_span(double v, double depth, double s, int n, int *lo, int *hi) {
  const int a = d2d_seen_cell(v - depth, s, n) - 1, b = d2d_seen_cell(v + depth, s, n) + 1;
  *lo = a < 0 ? 0 : a;
  *hi = b > n - 1 ? n - 1 : b;
}

/* does this call newly cover a cell whose record was `prev`?  (never seen, or not seen by the call before) */
D2D_SEEN_QUAL int d2d_seen_fresh(int prev, int call) { return prev == 0 || prev < call - 1; }

/* np.float32 of the cell's value after call `call`: tab[0][call - seen] where it was seen, tab[1][call] where it never was */
D2D_SEEN_QUAL float d2d_seen_age(const double *tab, int tab_len, int call, int seen) {
  const int s = seen < call ? seen : call;
  return (float)(seen > 0 ? tab[call - s] : tab[(size_t)tab_len + call]);
}

/* is there anything to do for an env whose counter says `steps` and whose latest update was `last`? */
D2D_SEEN_QUAL int d2d_seen_due(int steps, int last, int tab_len) {
  return steps >= 0 && steps + 1 > last && steps + 1 < tab_len;
}

/* the argument checks of d2d_seen_update: 0 or the error, `*why` the text */
D2D_SEEN_CHECK_QUAL int d2d_seen_check(const d2d_cfg *c, const d2d_state *s, const d2d_seen *w, const char **why) {
  *why = "";
  if (!c || !s || !w) return (*why = "d2d_seen_update: cfg, state or seen is NULL"), -1;
  if (c->abi_version != D2D_ABI_VERSION) return (*why = "d2d_seen_update: the cfg has another D2D_ABI_VERSION"), -2;
  if (!s->drone || !s->counters) return (*why = "d2d_seen_update: drone or counters is NULL"), -1;
  if (!w->seen || !w->last_call || !w->refreshed || !w->obs || !w->tab) return (*why = "d2d_seen_update: a seen buffer is NULL"), -1;
  if (c->B < 0 || c->W < 1 || c->H < 1 || c->L < 1 || !(c->scale > 0.0) || !(c->depth >= 0.0) || w->tab_len < 2)
    return (*why = "d2d_seen_update: B >= 0, W, H, L >= 1, scale > 0, depth >= 0, tab_len >= 2"), -1;
  if ((long long)c->W * c->H > 0x7fffffffll || (long long)c->L * c->L > 0x7fffffffll)
    return (*why = "d2d_seen_update: W * H and L * L are 32-bit cell indices"), -4;
  return 0;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_seen_update as a plain loop over host arrays (tests/csrc/seen_host.c), same layouts ---- */
D2D_SEEN_QUAL int d2d_seen_update_seq(const d2d_cfg *c, const d2d_state *s, const d2d_seen *w) {
  const char *why;
  const int rc = d2d_seen_check(c, s, w, &why);
  if (rc) return rc;
  const int W = c->W, H = c->H, L = c->L, edge = (L - 1) / 2;
  const double depth2 = c->depth * c->depth;
  for (size_t e = 0; e < (size_t)c->B; ++e) {
    const int steps = s->counters[e * D2D_CF + D2D_C_STEPS];
    if (!d2d_seen_due(steps, w->last_call[e], w->tab_len)) continue;
    const int call = steps + 1;
    const double *dr = s->drone + e * D2D_DF;
    const double x0 = dr[D2D_D_X], y0 = dr[D2D_D_Y];
    double cy, sy;
    d2d_seen_dir(dr[D2D_D_YAW], &cy, &sy);
    int32_t *seen = w->seen + e * (size_t)W * H;
    int i_lo, i_hi, j_lo, j_hi, fresh = 0;
    d2d_seen_span(x0, c->depth, c->scale, W, &i_lo, &i_hi);
    d2d_seen_span(y0, c->depth, c->scale, H, &j_lo, &j_hi);
    for (int i = i_lo; i <= i_hi; ++i)
      for (int j = j_lo; j <= j_hi; ++j)
        if (d2d_seen_view(w->acos_key_lo, w->acos_mask, depth2, x0, y0, cy, sy, (double)i * c->scale, (double)j * c->scale)) {
          fresh += d2d_seen_fresh(seen[i * H + j], call);
          seen[i * H + j] = call;
        }
    const int i0 = d2d_seen_cell(x0, c->scale, W) - edge, j0 = d2d_seen_cell(y0, c->scale, H) - edge;
    float *ob = w->obs + e * (size_t)L * L;
    for (int a = 0; a < L; ++a)
      for (int b = 0; b < L; ++b) {
        const int i = i0 + a, j = j0 + b;
        ob[a * L + b] = (i >= 0 && i < W && j >= 0 && j < H) ? d2d_seen_age(w->tab, w->tab_len, call, seen[i * H + j]) : 0.0f;
      }
    w->refreshed[e] = fresh;
    w->last_call[e] = call;
  }
  return 0;
}
#endif

#endif /* D2D_SEEN_IMPL_H */
