// d2d_scan.hip — the per-ray scan of the limited-FOV raycast on the device (gfx950): the kernel + the C entry points of
// include/d2d_scan.h.  Its own library (libd2d_scan.so): it shares no kernel with the step, the closed loop, the worlds, the metrics,
// the RVO profile, the Jerk_Primitive planner, the step path's gaze decision or the time-since-observed map.
//
//   scan_update   one wave per env, one wave a workgroup (so the barrier below is the wave's own).
//                 gate     the env's step counter and the counter of its latest update are requested together: an env that is not due
//                          (fresh, finished, or updated already) ends there, before it reads anything else, and writes nothing.
//                 cull     lane = agent, 64 a pass: the agents whose circle can hold a sample of this drone's rays (the distance bound
//                          of d2d_scan_near, no cone test) are compacted by ballots into an LDS list of D2D_SCAN_CCAP; an env with more
//                          of them tests every agent from global memory.
//                 march    lane = ray, ceil(R / 64) passes: d2d_scan_ray of d2d_scan.h, the reference's loop sample by sample.  Every
//                          ray writes its own end, kind, hit words and the two observation values; nothing is shared, no atomics.
//                 lane 0 writes last_step.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_scan.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_SCAN_QUAL __device__ __forceinline__
#define D2D_TAN_QUAL __device__ __forceinline__
#define D2D_TAN_TBL_QUAL __device__ const
#include "d2d_scan.h"

#define WAVE 64

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

__global__ __launch_bounds__(WAVE) void scan_update_kernel(const d2d_cfg c, const double *__restrict__ agents,
                                                           const uint8_t *__restrict__ gt, const int32_t *__restrict__ counters,
                                                           const d2d_scan w, const size_t grid_bytes) {
  __shared__ double s_cx[D2D_SCAN_CCAP], s_cy[D2D_SCAN_CCAP], s_cr2[D2D_SCAN_CCAP];
  __shared__ int32_t s_idx[D2D_SCAN_CCAP];
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;  // the grid is B workgroups

  // ---- gate ----
  const int steps = counters[e * D2D_CF + D2D_C_STEPS];
  const int last = w.last_step[e];
  if (!d2d_scan_due(steps, last)) return;  // uniform over the workgroup

  const double *pose = w.pose + e * D2D_DF;
  const double x0 = pose[D2D_D_X], y0 = pose[D2D_D_Y], yaw = pose[D2D_D_YAW];
  const int N = c.N, R = c.R, hw = w.hit_words;
  const double ss = c.scale - 1.0;
  const double *ag = agents + e * D2D_AF * (size_t)N;
  const double *ax = ag + (size_t)D2D_A_PX * N, *ay = ag + (size_t)D2D_A_PY * N, *ar2 = ag + (size_t)D2D_A_R2 * N;

  // ---- cull ----
  int ncand = 0;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    bool cand = false;
    double px = 0.0, py = 0.0, r2 = 0.0;
    if (k < N) {
      px = ax[k];
      py = ay[k];
      r2 = ar2[k];
      cand = d2d_scan_near(px, py, r2, x0, y0, c.depth, ss) != 0;
    }
    const unsigned long long m = __ballot(cand);
    const int slot = ncand + __popcll(m & ((1ull << lane) - 1ull));
    if (cand && slot < D2D_SCAN_CCAP) {
      s_cx[slot] = px;
      s_cy[slot] = py;
      s_cr2[slot] = r2;
      s_idx[slot] = k;
    }
    ncand += __popcll(m);
  }
  __syncthreads();

  d2d_scan_view v;
  if (ncand <= D2D_SCAN_CCAP) {
    v.cx = s_cx; v.cy = s_cy; v.cr2 = s_cr2; v.cidx = s_idx; v.ncand = ncand;
  } else {  // a crowd: every agent, as utils.py:658-662 does
    v.cx = ax; v.cy = ay; v.cr2 = ar2; v.cidx = nullptr; v.ncand = N;
  }
  v.W = c.W; v.H = c.H; v.tile = c.grid_tile;
  v.gt = gt + e * grid_bytes;
  v.scale = c.scale; v.W_px = c.W_px; v.H_px = c.H_px;
  v.depth2 = c.depth * c.depth;
  v.x0 = x0; v.y0 = y0;
  v.max_samples = d2d_scan_max_samples(c.W_px, c.H_px, ss);

  // ---- march ----
  float *ob = w.obs + e * 2 * (size_t)R;
  for (int i = lane; i < R; i += WAVE) {  // a lane past R forms no address at all
    double xs, ys;
    d2d_scan_steps(yaw, c.ray_off0, c.ray_dth, i, ss, &xs, &ys);
    const size_t ray = e * (size_t)R + (size_t)i;
    d2d_scan_ray(&v, xs, ys, hw, w.end + ray * 2, w.kind + ray, w.hit + ray * (size_t)hw, ob + i, ob + R + i);
  }
  if (lane == 0) w.last_step[e] = steps;
}

}  // namespace

extern "C" {

int d2d_scan_version(void) { return D2D_SCAN_VERSION; }
const char *d2d_scan_last_error(void) { return g_err; }

int d2d_scan_update(const d2d_cfg *c, const d2d_state *s, const d2d_scan *w, void *stream) {
  const char *why;
  const int rc = d2d_scan_check(c, s, w, &why);
  if (rc) return fail(rc, why);
  if (c->B == 0) return 0;
  hipLaunchKernelGGL(scan_update_kernel, dim3((unsigned)c->B), dim3(WAVE), 0, (hipStream_t)stream, *c, (const double *)s->agents,
                     (const uint8_t *)s->gt, (const int32_t *)s->counters, *w, D2D_GRID_BYTES(c));
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "d2d_scan_update: launch failed: %s", hipGetErrorString(err));
  return -3;
}

}  // extern "C"
