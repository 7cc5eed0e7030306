/*
 * d2d_render.h — the renderer's arithmetic, said once for the device kernels (d2d_render.hip) and for host builds
 * (tests/csrc/render_host_main.c): the numbers of every display-list item, an item's pixel box, the coverage rules and the work of one
 * lane of the rasteriser.  include/d2d_render.h states what each computes and names the reference lines.
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' below is one IEEE-754 binary64 operation.  There is no division and no
 * transcendental behind d2d_render_covers; the divisions of d2d_render_run_cells are one pair per run of pixels.
 */
#ifndef D2D_RENDER_IMPL_H
#define D2D_RENDER_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d_render.h"
#include "../../../include/d2d_render_hooks.h"

#ifndef D2D_RENDER_QUAL
#define D2D_RENDER_QUAL static inline
#endif
#ifndef D2D_RENDER_CHECK_QUAL
#define D2D_RENDER_CHECK_QUAL static inline /* the argument checks run on the host in every build */
#endif
#ifndef D2D_SINCOS_QUAL
#define D2D_SINCOS_QUAL D2D_RENDER_QUAL
#endif
#include "../d2d_sincos.h"

#define D2D_RENDER_TILE_W 128     /* frame pixels a workgroup covers: 32 rows of 8 runs */
#define D2D_RENDER_TILE_H 32
#define D2D_RENDER_RUN 16         /* consecutive frame pixels of one row a lane owns: 48 bytes */
#define D2D_RENDER_LDS_ITEMS 128  /* items a workgroup keeps per pass */
#define D2D_RENDER_ITEM_F64 22    /* sizeof(d2d_render_item) / 8 */
#define D2D_RENDER_DEG (0x1.921fb54442d18p+1 / 180.0) /* Python's degToRad = pi / 180 */

/* math.radians */
D2D_RENDER_QUAL double d2d_render_radians(double a) { return a * D2D_RENDER_DEG; }

/* what one slot's list is made from */
typedef struct d2d_render_src {
  const double *drone;    /* [D2D_DF] */
  const double *agents;   /* [D2D_AF][N] */
  const uint8_t *active;  /* [N] */
  const double *vel;      /* [2][N] or NULL */
  const double *target;   /* [2] */
  const int32_t *pillars; /* [P][3] */
  const double *traj;     /* position i at traj[i * traj_stride], + 1 */
  const double *star;     /* [10][2] sin, cos */
  int32_t traj_stride, traj_len, N, P, n_seeded, steps;
  double R, range, drone_radius;
} d2d_render_src;

/* the items of a slot: D2D_RENDER_FIXED + P + 2 N + the trajectory's segments */
D2D_RENDER_QUAL int d2d_render_total(const d2d_render_src *s) {
  return D2D_RENDER_FIXED + s->P + 2 * s->N + (s->traj_len > 1 ? s->traj_len - 1 : 0);
}

D2D_RENDER_QUAL void d2d_render_head(d2d_render_item *it, int kind, int r, int g, int b, double width, int npts) {
  it->kind = kind;
  it->rgb[0] = (uint8_t)r; it->rgb[1] = (uint8_t)g; it->rgb[2] = (uint8_t)b;
  it->npts = (uint8_t)npts;
  it->width = width;
  for (int i = 0; i < D2D_RENDER_GEOM; ++i) it->geom[i] = 0.0;
}

D2D_RENDER_QUAL void d2d_render_line(d2d_render_item *it, int grey, double ax, double ay, double bx, double by) {
  d2d_render_head(it, D2D_RK_LINE, grey, grey, grey, 2.0, 0);
  it->geom[0] = ax; it->geom[1] = ay; it->geom[2] = bx; it->geom[3] = by;
}

D2D_RENDER_QUAL void d2d_render_disc(d2d_render_item *it, int r, int g, int b, double cx, double cy, double rad) {
  d2d_render_head(it, D2D_RK_DISC, r, g, b, 0.0, 0);
  it->geom[0] = cx; it->geom[1] = cy; it->geom[2] = rad;
}

/* item i of the slot's list, 0 <= i < d2d_render_total(s) */
D2D_RENDER_QUAL void d2d_render_make(const d2d_render_src *s, int i, d2d_render_item *it) {
  const double x = s->drone[D2D_D_X], y = s->drone[D2D_D_Y], yaw = s->drone[D2D_D_YAW];
  if (i < 9) {
    const double half = s->range / 2;
    const double start = d2d_render_radians(yaw - half), stop = d2d_render_radians(yaw + half);
    if (i == 0) {
      d2d_render_head(it, D2D_RK_ARC, 100, 100, 100, 2.0, 0);
      it->geom[0] = x - s->R; it->geom[1] = y - s->R; it->geom[2] = 2 * s->R; it->geom[3] = 2 * s->R;
      it->geom[4] = start; it->geom[5] = stop;
      it->geom[6] = d2d_cos(start); it->geom[7] = d2d_sin(start); it->geom[8] = d2d_cos(stop); it->geom[9] = d2d_sin(stop);
      it->geom[10] = s->range;
    } else if (i <= 2) {
      const double a = i == 1 ? stop : start;                  /* angle1 first (utils.py:797-800) */
      d2d_render_line(it, 100, x, y, x + s->R * d2d_cos(a), y - s->R * d2d_sin(a));
    } else {
      const double a45 = d2d_render_radians(yaw + 45);
      const double dx = 5 * d2d_cos(a45), dy = -5 * d2d_sin(a45);
      if (i == 3) d2d_render_line(it, 100, x - dx, y - dy, x + dx, y + dy);
      else if (i == 4) d2d_render_line(it, 100, x - dy, y + dx, x + dy, y - dx);
      else if (i == 5) d2d_render_disc(it, 100, 100, 100, __builtin_trunc(x - dx), __builtin_trunc(y - dy), 3.5);
      else if (i == 6) d2d_render_disc(it, 100, 100, 100, __builtin_trunc(x + dx), __builtin_trunc(y + dy), 3.5);
      else if (i == 7) d2d_render_disc(it, 100, 100, 100, __builtin_trunc(x - dy), __builtin_trunc(y + dx), 3.5);
      else d2d_render_disc(it, 100, 100, 100, __builtin_trunc(x + dy), __builtin_trunc(y - dx), 3.5);
    }
    return;
  }
  i -= 9;
  if (i < s->P) {
    const int32_t *p = s->pillars + (size_t)i * 3;
    d2d_render_disc(it, 130, 130, 130, (double)p[0], (double)p[1], (double)p[2]);
    return;
  }
  i -= s->P;
  const int nseg = s->traj_len > 1 ? s->traj_len - 1 : 0;
  if (i < nseg) {
    const double *a = s->traj + (size_t)i * s->traj_stride, *b = a + s->traj_stride;
    d2d_render_line(it, 0, a[0], a[1], b[0], b[1]);
    return;
  }
  i -= nseg;
  if (i < 2 * s->N) {
    const int k = i >> 1, N = s->N;
    const double px = s->agents[D2D_A_PX * N + k], py = s->agents[D2D_A_PY * N + k];
    const double cx = __builtin_rint(px), cy = __builtin_rint(py);
    if (!(i & 1)) {
      const int on = s->active[k] != 0;
      d2d_render_disc(it, on ? 130 : 200, on ? 176 : 36, on ? 210 : 35, cx, cy, __builtin_rint(s->agents[D2D_A_R * N + k]));
    } else {
      double vx, vy;
      if (s->vel) {
        vx = s->vel[k]; vy = s->vel[N + k];
      } else if (s->steps == 0 && k < s->n_seeded) {
        vx = 0.0; vy = 0.0;
      } else {
        vx = s->agents[D2D_A_VX * N + k]; vy = s->agents[D2D_A_VY * N + k];
      }
      d2d_render_line(it, 53, cx, cy, __builtin_rint(px + vx), __builtin_rint(py + vy));
    }
    return;
  }
  /* the star (utils.py:31-51): outer radius on the even points, inner on the odd ones */
  d2d_render_head(it, D2D_RK_POLY, 0, 0, 150, 0.0, 10);
  const double outer = s->drone_radius, inner = s->drone_radius * 0.5;
  for (int q = 0; q < 10; ++q) {
    const double rad = (q & 1) ? inner : outer;
    it->geom[2 * q] = s->target[0] + rad * s->star[2 * q];
    it->geom[2 * q + 1] = s->target[1] - rad * s->star[2 * q + 1];
  }
}

/* ---- the pixel box of an item: every pixel it can cover lies inside, cut to the frame; x0 > x1 where there is none ---- */
D2D_RENDER_QUAL int d2d_render_clampi(double v, int lo, int hi) {
  if (!(v >= (double)lo)) return lo; /* (NaN too) */
  if (v > (double)hi) return hi;
  return (int)v;
}

D2D_RENDER_QUAL void d2d_render_bbox(const d2d_render_item *it, int W_px, int H_px, int16_t *out) {
  double x0, y0, x1, y1, pad = 1.0;
  const double *g = it->geom;
  if (it->kind == D2D_RK_DISC) {
    x0 = g[0] - g[2]; x1 = g[0] + g[2]; y0 = g[1] - g[2]; y1 = g[1] + g[2];
  } else if (it->kind == D2D_RK_LINE) {
    x0 = g[0] < g[2] ? g[0] : g[2]; x1 = g[0] < g[2] ? g[2] : g[0];
    y0 = g[1] < g[3] ? g[1] : g[3]; y1 = g[1] < g[3] ? g[3] : g[1];
    pad = 1.0 + it->width * 0.5;
  } else if (it->kind == D2D_RK_ARC) {
    x0 = g[0]; x1 = g[0] + g[2]; y0 = g[1]; y1 = g[1] + g[3];
  } else if (it->kind == D2D_RK_POLY && it->npts >= 1 && it->npts <= 10) {
    x0 = x1 = g[0]; y0 = y1 = g[1];
    for (int q = 1; q < it->npts; ++q) {
      x0 = g[2 * q] < x0 ? g[2 * q] : x0; x1 = g[2 * q] > x1 ? g[2 * q] : x1;
      y0 = g[2 * q + 1] < y0 ? g[2 * q + 1] : y0; y1 = g[2 * q + 1] > y1 ? g[2 * q + 1] : y1;
    }
  } else {
    x0 = y0 = 1.0; x1 = y1 = 0.0; pad = 0.0;
  }
  int ok = x0 <= x1 && y0 <= y1; /* (false for a NaN) */
  x0 = __builtin_floor(x0 - pad); y0 = __builtin_floor(y0 - pad); x1 = __builtin_ceil(x1 + pad); y1 = __builtin_ceil(y1 + pad);
  ok = ok && x1 >= 0.0 && y1 >= 0.0 && x0 <= (double)(W_px - 1) && y0 <= (double)(H_px - 1);
  out[0] = (int16_t)(ok ? d2d_render_clampi(x0, 0, W_px - 1) : 1);
  out[1] = (int16_t)(ok ? d2d_render_clampi(y0, 0, H_px - 1) : 1);
  out[2] = (int16_t)(ok ? d2d_render_clampi(x1, 0, W_px - 1) : 0);
  out[3] = (int16_t)(ok ? d2d_render_clampi(y1, 0, H_px - 1) : 0);
}

/* does the box reach into the pixels [tx0, tx1] x [ty0, ty1]? */
D2D_RENDER_QUAL int d2d_render_box_hits(const int16_t *b, int tx0, int ty0, int tx1, int ty1) {
  return b[0] <= b[2] && b[0] <= tx1 && b[2] >= tx0 && b[1] <= ty1 && b[3] >= ty0;
}

/* ---- the coverage rules (include/d2d_render.h) ---- */
D2D_RENDER_QUAL int d2d_render_in_disc(double x, double y, double cx, double cy, double r2) {
  const double dx = x - cx, dy = y - cy;
  return dx * dx + dy * dy <= r2;
}

D2D_RENDER_QUAL int d2d_render_covers(const d2d_render_item *it, double x, double y) {
  const double *g = it->geom;
  switch (it->kind) {
    case D2D_RK_DISC:
      return d2d_render_in_disc(x, y, g[0], g[1], g[2] * g[2]);
    case D2D_RK_LINE: {
      const double h = it->width * 0.5, h2 = h * h;
      const double apx = x - g[0], apy = y - g[1], abx = g[2] - g[0], aby = g[3] - g[1];
      const double t = apx * abx + apy * aby, l2 = abx * abx + aby * aby;
      if (l2 == 0.0 || t <= 0.0) return d2d_render_in_disc(x, y, g[0], g[1], h2);
      if (t >= l2) return d2d_render_in_disc(x, y, g[2], g[3], h2);
      const double c = abx * apy - aby * apx;
      return c * c <= h2 * l2;
    }
    case D2D_RK_ARC: {
      const double R = g[2] * 0.5, cx = g[0] + R, cy = g[1] + g[3] * 0.5;
      const double dx = x - cx, ey = -(y - cy), q = dx * dx + ey * ey;
      double ri = R - it->width;
      if (ri < 0.0) ri = 0.0;
      if (!(ri * ri <= q && q <= R * R)) return 0;
      if (g[10] >= 360.0) return 1;
      const int left = g[6] * ey - g[7] * dx >= 0.0, right = g[8] * ey - g[9] * dx <= 0.0;
      return g[10] <= 180.0 ? (left && right) : (left || right);
    }
    case D2D_RK_POLY: {
      const int n = it->npts;
      int in = 0;
      if (n < 3 || n > 10) return 0;
      for (int i = 0, j = n - 1; i < n; j = i++) {
        const double xi = g[2 * i], yi = g[2 * i + 1], xj = g[2 * j], yj = g[2 * j + 1];
        if ((yi > y) != (yj > y)) {
          const double dy = yj - yi, lhs = (x - xi) * dy, rhs = (xj - xi) * (y - yi);
          if (dy > 0.0 ? lhs < rhs : lhs > rhs) in ^= 1;
        }
      }
      return in;
    }
    default:
      return 0;
  }
}

/* ---- the cell layer ---- */
D2D_RENDER_QUAL uint32_t d2d_render_cell_rgb(uint8_t code) {
  const uint32_t v = code == D2D_OCCUPIED ? 100u : (code == D2D_UNOCCUPIED || code == D2D_DYNAMIC) ? 200u : 240u;
  return v | (v << 8) | (v << 16);
}

D2D_RENDER_QUAL size_t d2d_render_cell_at(int i, int j, int H, int tile) {
  if (!tile) return (size_t)i * (size_t)H + (size_t)j;
  return ((size_t)(i >> 4) * (size_t)((H + 15) >> 4) + (size_t)(j >> 4)) * 256 + (size_t)((i & 15) * 16 + (j & 15));
}

/* one lane's run of n <= D2D_RENDER_RUN frame pixels of the full-resolution row y, the first at x0, d apart: px[p] = the cell
 * layer's colour as 0x00bbggrr.  A pixel beyond the last cell (a map size that is no multiple of the scale) is UNEXPLORED.
 * One division pair for the run; the cell index then moves by additions */
D2D_RENDER_QUAL void d2d_render_run_cells(const uint8_t *grid, int W, int H, int tile, int scale, int x0, int y, int d, int n,
                                          uint32_t *px) {
  const int j = y / scale;
  int i = x0 / scale, rem = x0 - i * scale, last = -1;
  uint32_t colour = 0;
  for (int p = 0; p < D2D_RENDER_RUN; ++p) {
    if (p < n) {
      if (i != last) {
        colour = d2d_render_cell_rgb(i < W && j < H ? grid[d2d_render_cell_at(i, j, H, tile)] : (uint8_t)D2D_UNEXPLORED);
        last = i;
      }
      px[p] = colour;
      rem += d;
      while (rem >= scale) {
        rem -= scale;
        ++i;
      }
    }
  }
}

/* the same run under the nk kept items (records `kept`, their boxes `kbox`), in their order: the last one that covers a pixel wins */
D2D_RENDER_QUAL void d2d_render_run_items(const d2d_render_item *kept, const int16_t *kbox, int nk, int x0, int y, int d, int n,
                                          uint32_t *px) {
  const int x1 = x0 + (n - 1) * d;
  const double fy = (double)y;
  for (int k = 0; k < nk; ++k) {
    const int16_t *b = kbox + 4 * k;
    if (y < b[1] || y > b[3] || x1 < b[0] || x0 > b[2]) continue;
    const d2d_render_item *it = kept + k;
    const uint32_t colour = (uint32_t)it->rgb[0] | ((uint32_t)it->rgb[1] << 8) | ((uint32_t)it->rgb[2] << 16);
    for (int p = 0; p < D2D_RENDER_RUN; ++p)
      if (p < n && d2d_render_covers(it, (double)(x0 + p * d), fy)) px[p] = colour;
  }
}

/* what d2d_render_frame and d2d_render_raster take of a geometry: 0 or the error, `*why` the text */
D2D_RENDER_CHECK_QUAL int d2d_render_check_geometry(long long S, int cap, int W, int H, int W_px, int H_px, int scale, int d, const char **why) {
  *why = "";
  if (S < 0 || cap < 1 || W < 1 || H < 1 || W_px < 1 || H_px < 1 || scale < 1) return (*why = "d2d_render: S >= 0, cap, W, H, W_px, H_px, scale >= 1"), -1;
  if (d < 1 || d > D2D_RENDER_MAX_DOWNSAMPLE) return (*why = "d2d_render: downsample is 1 .. 64"), -1;
  if (W_px > 32767 || H_px > 32767) return (*why = "d2d_render: a frame of more than 32767 pixels a side (the item boxes are 16-bit)"), -4;
  const long long Wf = (W_px + d - 1) / d, Hf = (H_px + d - 1) / d;
  const long long tiles = ((Wf + D2D_RENDER_TILE_W - 1) / D2D_RENDER_TILE_W) * ((Hf + D2D_RENDER_TILE_H - 1) / D2D_RENDER_TILE_H);
  if (S > 0 && tiles > 0x7fffffffll / S) return (*why = "d2d_render: more than 2^31 - 1 workgroups"), -4;
  if (S > 0 && (long long)cap > 0x7fffffffll / S) return (*why = "d2d_render: S * cap is a 32-bit index"), -4;
  return 0;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- d2d_render_raster as plain loops over host arrays: the kernel's tiles, passes and runs one after the other ---- */
D2D_RENDER_QUAL int d2d_render_raster_seq(const d2d_render_raster_call *c) {
  const char *why;
  if (!c) return -1;
  const int rc = d2d_render_check_geometry(c->S, c->cap, c->W, c->H, c->W_px, c->H_px, c->scale, c->downsample, &why);
  if (rc) return rc;
  if (c->S && (!c->items || !c->count || !c->cells || !c->bbox || !c->frame)) return -1;
  const int d = c->downsample, Wf = (c->W_px + d - 1) / d, Hf = (c->H_px + d - 1) / d;
  d2d_render_item kept[D2D_RENDER_LDS_ITEMS];
  int16_t kbox[D2D_RENDER_LDS_ITEMS * 4];
  for (int k = 0; k < c->S; ++k) {
    const d2d_render_item *items = c->items + (size_t)k * c->cap;
    int16_t *bbox = c->bbox + (size_t)k * c->cap * 4;
    const uint8_t *grid = c->cells + (size_t)k * c->W * c->H;
    uint8_t *frame = c->frame + (size_t)k * Hf * Wf * 3;
    int count = c->count[k];
    if (count < 0) count = 0;
    if (count > c->cap) count = c->cap;
    for (int i = 0; i < count; ++i) d2d_render_bbox(items + i, c->W_px, c->H_px, bbox + 4 * i);
    for (int tv = 0; tv < Hf; tv += D2D_RENDER_TILE_H)
      for (int tu = 0; tu < Wf; tu += D2D_RENDER_TILE_W) {
        const int tx0 = tu * d, ty0 = tv * d, tx1 = (tu + D2D_RENDER_TILE_W - 1) * d, ty1 = (tv + D2D_RENDER_TILE_H - 1) * d;
        for (int c0 = 0; c0 == 0 || c0 < count; c0 += D2D_RENDER_LDS_ITEMS) {
          int nk = 0;
          for (int i = c0; i < count && i < c0 + D2D_RENDER_LDS_ITEMS; ++i)
            if (d2d_render_box_hits(bbox + 4 * i, tx0, ty0, tx1, ty1)) {
              kept[nk] = items[i];
              for (int q = 0; q < 4; ++q) kbox[4 * nk + q] = bbox[4 * i + q];
              ++nk;
            }
          for (int v = tv; v < tv + D2D_RENDER_TILE_H && v < Hf; ++v)
            for (int u0 = tu; u0 < tu + D2D_RENDER_TILE_W && u0 < Wf; u0 += D2D_RENDER_RUN) {
              const int n = Wf - u0 < D2D_RENDER_RUN ? Wf - u0 : D2D_RENDER_RUN;
              uint32_t px[D2D_RENDER_RUN];
              uint8_t *out = frame + ((size_t)v * Wf + u0) * 3;
              if (c0 == 0) d2d_render_run_cells(grid, c->W, c->H, 0, c->scale, u0 * d, v * d, d, n, px);
              else
                for (int p = 0; p < n; ++p) px[p] = (uint32_t)out[3 * p] | ((uint32_t)out[3 * p + 1] << 8) | ((uint32_t)out[3 * p + 2] << 16);
              d2d_render_run_items(kept, kbox, nk, u0 * d, v * d, d, n, px);
              for (int p = 0; p < n; ++p) {
                out[3 * p] = (uint8_t)px[p]; out[3 * p + 1] = (uint8_t)(px[p] >> 8); out[3 * p + 2] = (uint8_t)(px[p] >> 16);
              }
            }
        }
      }
  }
  return 0;
}

/* ---- one slot's display list as a plain loop: count, or -1 where it does not fit cap (nothing is written then) ---- */
D2D_RENDER_QUAL int d2d_render_list_seq(const d2d_render_src *s, int cap, d2d_render_item *items) {
  const int total = d2d_render_total(s);
  if (total > cap) return -1;
  for (int i = 0; i < total; ++i) d2d_render_make(s, i, items + i);
  return total;
}
#endif

#endif /* D2D_RENDER_IMPL_H */
