// d2d_seen.hip — the time-since-observed map as an observation channel on the device (gfx950): the kernel + the C entry points of
// include/d2d_seen.h.  Its own library (libd2d_seen.so): it shares no kernel with the step, the closed loop, the worlds, the metrics,
// the RVO profile, the Jerk_Primitive planner or the step path's gaze decision.
//
//   seen_update   one wave per env, four envs a workgroup, no LDS.
//                 gate     the env's step counter and the call of its latest update are requested together: an env that is not due
//                          (finished, stepped past the table, or updated already) ends there and writes nothing.
//                 mark     lane = cell of the box around the drone, 64 cells a pass: the view test, the cell's previous record read by
//                          the lane that then writes it; the newly covered cells are counted by ballots.
//                 crop     lane = cell of the L x L window, 64 a pass: the record of a cell inside the map, overruled by the view test
//                          for the cells this launch marks (no lane reads back what another lane wrote), the table value as float32.
//                 lane 0 writes refreshed and last_call.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_seen.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_SEEN_QUAL __device__ __forceinline__
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#include "d2d_seen.h"

#define WAVE 64
#define SEEN_WAVES 4

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

__global__ __launch_bounds__(SEEN_WAVES *WAVE) void seen_update_kernel(const d2d_cfg c, const double *__restrict__ drone,
                                                                      const int32_t *__restrict__ counters, const d2d_seen w) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long e = (long long)blockIdx.x * SEEN_WAVES + (threadIdx.x >> 6);
  if (e >= c.B) return;

  // ---- gate: one batch of loads ----
  const int steps = counters[(size_t)e * D2D_CF + D2D_C_STEPS];
  const int last = w.last_call[e];
  const double *dr = drone + (size_t)e * D2D_DF;
  const double x0 = dr[D2D_D_X], y0 = dr[D2D_D_Y], yaw = dr[D2D_D_YAW];
  if (!d2d_seen_due(steps, last, w.tab_len)) return;
  const int call = steps + 1;

  const int W = c.W, H = c.H, L = c.L, edge = (L - 1) / 2;
  const double depth2 = c.depth * c.depth;
  double cy, sy;
  d2d_seen_dir(yaw, &cy, &sy);
  int32_t *seen = w.seen + (size_t)e * W * H;

  // ---- mark: the cells the pose sees (yaw_planner.py:92-97); only the box around the drone can be seen ----
  int i_lo, i_hi, j_lo, j_hi, fresh = 0;
  d2d_seen_span(x0, c.depth, c.scale, W, &i_lo, &i_hi);
  d2d_seen_span(y0, c.depth, c.scale, H, &j_lo, &j_hi);
  const int nc = j_hi - j_lo + 1, nsub = (i_hi - i_lo + 1) * nc;  // (at most (2 depth / scale + 5) ** 2, and no more than W * H)
  if (nc > 0 && nsub > 0) {
    for (int q0 = 0; q0 < nsub; q0 += WAVE) {
      const int q = q0 + lane;
      bool marked = false;
      int prev = 0;
      if (q < nsub) {
        const int r = q / nc, i = i_lo + r, j = j_lo + (q - r * nc);  // i in [i_lo, i_hi], j in [j_lo, j_hi]: inside the map
        marked = d2d_seen_view(w.acos_key_lo, w.acos_mask, depth2, x0, y0, cy, sy, (double)i * c.scale, (double)j * c.scale) != 0;
        if (marked) {
          prev = seen[i * H + j];
          seen[i * H + j] = call;
        }
      }
      fresh += __popcll(__ballot(marked && d2d_seen_fresh(prev, call)));
    }
  }

  // ---- crop: the L x L window around the drone's cell, zero outside the map ----
  const int i0 = d2d_seen_cell(x0, c.scale, W) - edge, j0 = d2d_seen_cell(y0, c.scale, H) - edge;
  float *__restrict__ ob = w.obs + (size_t)e * L * L;
  const int nn = L * L;
  for (int idx = lane; idx < nn; idx += WAVE) {
    const int a = idx / L, i = i0 + a, j = j0 + (idx - a * L);
    float v = 0.0f;
    if (i >= 0 && i < W && j >= 0 && j < H) {
      int sn = seen[i * H + j];
      // a cell marked above: decided here again, whichever of the two values the load returned
      if (d2d_seen_view(w.acos_key_lo, w.acos_mask, depth2, x0, y0, cy, sy, (double)i * c.scale, (double)j * c.scale)) sn = call;
      v = d2d_seen_age(w.tab, w.tab_len, call, sn);
    }
    ob[idx] = v;
  }
  if (lane == 0) {
    w.refreshed[e] = fresh;
    w.last_call[e] = call;
  }
}

}  // namespace

extern "C" {

int d2d_seen_version(void) { return D2D_SEEN_VERSION; }
const char *d2d_seen_last_error(void) { return g_err; }

int d2d_seen_update(const d2d_cfg *c, const d2d_state *s, const d2d_seen *w, void *stream) {
  const char *why;
  const int rc = d2d_seen_check(c, s, w, &why);
  if (rc) return fail(rc, why);
  if (c->B == 0) return 0;
  hipLaunchKernelGGL(seen_update_kernel, dim3((unsigned)(((long long)c->B + SEEN_WAVES - 1) / SEEN_WAVES)), dim3(SEEN_WAVES * WAVE), 0,
                     (hipStream_t)stream, *c, (const double *)s->drone, (const int32_t *)s->counters, *w);
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "d2d_seen_update: launch failed: %s", hipGetErrorString(err));
  return -3;
}

}  // extern "C"
