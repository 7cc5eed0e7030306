/*
 * d2d_difficulty.h — per-element arithmetic of the traversability and survival-fit difficulty metrics (include/d2d_metrics.h
 * names the reference lines).
 *
 * Traversability (demos/traversibility.py:26-51): from a start cell of the ground-truth grid, a walk in one of eight directions
 * goes on while the next cell is inside the grid and UNOCCUPIED (2).  The device and the loops below count STEPS (integers); the
 * host turns them into the reference's floats (a straight step 1, a diagonal one math.sqrt(2), added one at a time).
 *
 * Survival fit (script/difficulty_calculator/survivability_calculator.py:13-48): the agents move under the constant-velocity
 * model (envs/drone_v2.py:176-179 + utils.py:472-493) and a drone of radius rd standing at `pos` is hit by agent j when
 *
 *   numpy.linalg.norm(agent.position - pos) < agent.radius + rd      norm of a 2-vector = sqrt(fma(y, y, x * x)) (d2d_vo.h)
 *
 * One agent update, every step:
 *
 *   velocity      = pref_velocity                 the SAME array: what the bounces write into pref_velocity moves the agent in
 *                                                 this very step ...
 *   new_position  = position + velocity * dt
 *   norm(velocity) <= 5  ->  pref_velocity = R(pi/6) @ pref_velocity      ... unless the stuck-agent rotation has just replaced
 *                                                 pref_velocity by a new array: then the step moves by the old velocity
 *   new_position.x <  scale + r          -> pref_velocity.x =  |pref_velocity.x|
 *   new_position.x >  W_px - scale - r   -> pref_velocity.x = -|pref_velocity.x|      (likewise y against H_px)
 *   position      = position + velocity * dt
 *
 * It is the arithmetic of the step library's agent stage, restated here because this library shares no code with it.
 *
 * The scalar pieces are shared by the device kernels (d2d_metrics.hip) and by the plain loops at the end of this file (host
 * builds only), which the CPU tests compare with a Python model.  Must be compiled with -ffp-contract=off: every '*' '+' '-' is
 * one IEEE-754 binary64 operation, every __builtin_fma one fused multiply-add (numpy's norm and its 2x2 @ 2x1 product).
 */
#ifndef D2D_DIFFICULTY_IMPL_H
#define D2D_DIFFICULTY_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d.h" /* D2D_AF, D2D_A_*: the rows of the state's agents [6][N] */
#include "../../../include/d2d_metrics.h"

#ifndef D2D_DF_QUAL
#define D2D_DF_QUAL static inline
#endif

#define D2D_DF_UNOCCUPIED 2

/* direction d of demos/traversibility.py:5-14 on grid[i][j]: N, NE, E, SE, S, SW, W, NW */
D2D_DF_QUAL int d2d_trav_di(int d) { return d == 0 || d == 1 || d == 7 ? -1 : (d >= 3 && d <= 5 ? 1 : 0); }
D2D_DF_QUAL int d2d_trav_dj(int d) { return d >= 1 && d <= 3 ? 1 : (d >= 5 ? -1 : 0); }

/* demos/traversibility.py:35-48 for one direction: the steps walked from (i, j) over grid [W][H] (row-major, grid[i * H + j]).
 * (i, j) must lie inside the grid; no cell outside it is read. */
D2D_DF_QUAL int32_t d2d_trav_ray(const uint8_t *grid, int W, int H, int i, int j, int d) {
  const int di = d2d_trav_di(d), dj = d2d_trav_dj(d);
  int32_t steps = 0;
  for (;;) {
    i += di;
    j += dj;
    if (i < 0 || j < 0 || i >= W || j >= H) break;
    if (grid[(size_t)i * H + j] != D2D_DF_UNOCCUPIED) break;
    ++steps;
  }
  return steps;
}

/* 1 iff start (i, j) is a cell of the grid and UNOCCUPIED (traversibility.py:32 returns 0 for any other cell) */
D2D_DF_QUAL int d2d_trav_open(const uint8_t *grid, int W, int H, int i, int j) {
  return i >= 0 && j >= 0 && i < W && j < H && grid[(size_t)i * H + j] == D2D_DF_UNOCCUPIED;
}

/* One update of one agent under the constant-velocity model: (px, py) the position, (vx, vy) pref_velocity, r the radius. */
D2D_DF_QUAL void d2d_fit_agent_step(double *px, double *py, double *vx, double *vy, double r, double W_px, double H_px, double scale,
                                    double dt) {
  const double cs = 0x1.bb67ae8584cabp-1, sn = 0x1.fffffffffffffp-2; /* cos(pi/6), sin(pi/6) as numpy returns them */
  const double velx = *vx, vely = *vy;
  const double nx = *px + velx * dt, ny = *py + vely * dt;
  int aliased = 1;
  double pvx = velx, pvy = vely;
  /* norm(v) <= 5: sqrt is correctly rounded and monotonic, and sqrt(s) rounds to <= 5 exactly for s <= nextafter(25) */
  if (__builtin_fma(vely, vely, velx * velx) <= 0x1.9000000000001p+4) {
    /* numpy 2x2 @ 2x1: fma(M[r][0], v0, M[r][1] * v1) */
    pvx = __builtin_fma(cs, velx, (-sn) * vely);
    pvy = __builtin_fma(sn, velx, cs * vely);
    aliased = 0;
  }
  if (nx < scale + r) pvx = __builtin_fabs(pvx);
  else if (nx > W_px - scale - r) pvx = -__builtin_fabs(pvx);
  if (ny < scale + r) pvy = __builtin_fabs(pvy);
  else if (ny > H_px - scale - r) pvy = -__builtin_fabs(pvy);
  const double ux = aliased ? pvx : velx, uy = aliased ? pvy : vely;
  *px = *px + ux * dt;
  *py = *py + uy * dt;
  *vx = pvx;
  *vy = pvy;
}

/* survivability_calculator.py:39 with rr = agent.radius + drone.radius: the agent at (bx, by) hits the drone at (ax, ay) */
D2D_DF_QUAL int d2d_fit_hits(double ax, double ay, double bx, double by, double rr) {
  const double x = bx - ax, y = by - ay;
  return __builtin_sqrt(__builtin_fma(y, y, x * x)) < rr;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- the two entry points as plain loops over host arrays (tests/csrc/difficulty_host.c), layouts of include/d2d_metrics.h ---- */

D2D_DF_QUAL void d2d_trav_steps_seq(const uint8_t *gt, int B, int W, int H, const int32_t *starts, int S, int32_t *steps) {
  for (int b = 0; b < B; ++b) {
    const uint8_t *g = gt + (size_t)b * W * H;
    for (int s = 0; s < S; ++s) {
      const int i = starts[2 * s], j = starts[2 * s + 1];
      const int open = d2d_trav_open(g, W, H, i, j);
      for (int d = 0; d < 8; ++d) steps[((size_t)b * S + s) * 8 + d] = open ? d2d_trav_ray(g, W, H, i, j, d) : -1;
    }
  }
}

/* `work`: 5 * N doubles of scratch */
D2D_DF_QUAL void d2d_fit_first_hit_seq(const double *agents, const double *pos, double drone_radius, double W_px, double H_px,
                                       double scale, double dt, int B, int N, int P, int checks, int32_t *first, double *agents_out,
                                       double *work) {
  double *px = work, *py = work + N, *vx = work + 2 * (size_t)N, *vy = work + 3 * (size_t)N, *rr = work + 4 * (size_t)N;
  for (int b = 0; b < B; ++b) {
    const double *ag = agents + (size_t)b * D2D_AF * N;
    for (int j = 0; j < N; ++j) {
      px[j] = ag[D2D_A_PX * N + j];
      py[j] = ag[D2D_A_PY * N + j];
      vx[j] = ag[D2D_A_VX * N + j];
      vy[j] = ag[D2D_A_VY * N + j];
      rr[j] = ag[D2D_A_R * N + j] + drone_radius;
    }
    for (int p = 0; p < P; ++p) first[(size_t)b * P + p] = -1;
    for (int k = -1; k < checks; ++k) {
      if (k >= 0)
        for (int p = 0; p < P; ++p) {
          int32_t *f = first + (size_t)b * P + p;
          for (int j = 0; j < N && *f < 0; ++j)
            if (d2d_fit_hits(pos[2 * p], pos[2 * p + 1], px[j], py[j], rr[j])) *f = k;
        }
      for (int j = 0; j < N; ++j) d2d_fit_agent_step(px + j, py + j, vx + j, vy + j, ag[D2D_A_R * N + j], W_px, H_px, scale, dt);
    }
    if (agents_out) {
      double *o = agents_out + (size_t)b * D2D_AF * N;
      for (int j = 0; j < N; ++j) {
        o[D2D_A_PX * N + j] = px[j];
        o[D2D_A_PY * N + j] = py[j];
        o[D2D_A_VX * N + j] = vx[j];
        o[D2D_A_VY * N + j] = vy[j];
        o[D2D_A_R * N + j] = ag[D2D_A_R * N + j];
        o[D2D_A_R2 * N + j] = ag[D2D_A_R2 * N + j];
      }
    }
  }
}
#endif

#endif /* D2D_DIFFICULTY_IMPL_H */
