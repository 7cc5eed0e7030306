// d2d_jerk.hip — the Jerk_Primitive planner on the device (gfx950): kernels + the C entry points of include/d2d_jerk.h.  Its own
// library (libd2d_jerk.so): it shares no kernel with the step, the closed loop, the worlds, the metrics or the RVO profile.
//
//   jerk_plan    one wave per env.
//                trackers    lane = tracker: the archive bookkeeping, and the active ones compacted into LDS as five planes
//                            (mu x, y, vx, vy, the distance limit), where every sample of every primitive reads them as broadcasts.
//                ranks       lane = heading (72 = 64 + 8): the cost, then its rank by (cost, index) from a walk over the 72 costs in
//                            LDS; then the host's tie table row for the goal's pattern, taken where it fits the costs at hand.
//                walk        passes in rank order, the lanes spread over (rank, sample) pairs: 64 / S primitives a pass (S > 64: one
//                            primitive in two passes).  Every lane derives the six coefficients of its own primitive (a few dozen
//                            operations; no exchange), takes its sample's position and tests it; one ballot per pass tells which
//                            primitives are free.  The first pass that holds a free primitive ends the walk: the reference is lazy,
//                            and an env whose best heading is free runs one pass.
//                tie flag    when the heading after the chosen one has the same cost, one more pass with lane = sample tests it.
//                Lane 0 recomputes the chosen primitive's first sample and writes the env's outputs.
//   jerk_plan_live  jerk_plan for a batch with finished envs (include/d2d_jerk_live.h): the body is shared as text
//                (d2d_jerk_wave.inc); the wave loads its env's done byte first and ends there if it is set.
//   jerk_reset   thread = (env, tracker).
//
// Arithmetic is fp64 in the reference's own operation order (d2d_jerk.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_JERK_QUAL __device__ __forceinline__
#define D2D_ATAN2_QUAL __device__ __forceinline__
#define D2D_ATAN2_TBL_QUAL __device__ const
#define D2D_POW2_QUAL __device__ __forceinline__
#define D2D_POW2_TBL_QUAL __device__ const
#include "d2d_jerk.h"
#include "../../../include/d2d_jerk_live.h"

#define WAVE 64
#define EW_BLOCK 256
#define NT D2D_JERK_NTHETA

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

__attribute__((format(printf, 2, 3))) int failf(int rc, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return rc;
}

// are all `times` samples of the primitive at heading `th` free?  lane = sample, 64 at a time (wave-uniform result)
__device__ __forceinline__ bool prim_free(const d2d_jerk_call &c, const d2d_jerk_env &e, int th, int lane) {
  const int times = d2d_jerk_times(&c, th);
  d2d_jerk_prim q;
  d2d_jerk_primitive(c.th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c.half_v_max, &q);
  for (int s0 = 0; s0 < times; s0 += WAVE) {
    const int s = s0 + lane;
    const bool bad = s < times && !d2d_jerk_sample_free(&c, &e, &q, th, s);
    if (__ballot(bad) != 0ull) return false;
  }
  return true;
}

__global__ __launch_bounds__(WAVE) void jerk_plan_kernel(const d2d_jerk_call c) {
#include "d2d_jerk_wave.inc"   // the body, shared as text with jerk_plan_live_kernel: this kernel compiles to what it always did
}

// the same for a batch with finished envs (include/d2d_jerk_live.h).  The done byte's address depends on blockIdx.x alone, so the test is
// uniform over the wave, which is the whole workgroup: a finished env's wave ends here, before the tracker loop (which writes
// trk_radius / trk_prev), before any LDS write and before the first __syncthreads()
__global__ __launch_bounds__(WAVE) void jerk_plan_live_kernel(const d2d_jerk_call c, const uint8_t *__restrict__ flags) {
  if (__builtin_amdgcn_readfirstlane(flags[(size_t)blockIdx.x * 4 + D2D_JERK_LIVE_F_DONE])) return;
#include "d2d_jerk_wave.inc"
}

__global__ __launch_bounds__(EW_BLOCK) void jerk_reset_kernel(double *__restrict__ trk_radius, uint8_t *__restrict__ trk_prev,
                                                             const double *__restrict__ trk_radius0, const uint8_t *__restrict__ mask,
                                                             int mask_stride, int N, long long total) {
  const long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (t >= total) return;
  if (mask && !mask[(size_t)(t / N) * mask_stride]) return;
  trk_radius[t] = trk_radius0[t];
  trk_prev[t] = 0;
}

int launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  return failf(-3, "%s: launch failed: %s", who, hipGetErrorString(err));
}

// what d2d_jerk_plan and d2d_jerk_plan_live refuse alike, under the name of the entry point
int check_call(const char *who, const d2d_jerk_call *c) {
  if (!c) return failf(-1, "%s: call is NULL", who);
  if (c->B < 1 || c->N < 0 || c->S < 1) return failf(-1, "%s: B >= 1, N >= 0, S >= 1", who);
  if (c->S > D2D_JERK_MAX_S) return failf(-4, "%s: S = %d samples a primitive, at most %d", who, c->S, D2D_JERK_MAX_S);
  if (c->N > D2D_JERK_MAX_N) return failf(-4, "%s: N = %d trackers, at most %d fit the wave's LDS", who, c->N, D2D_JERK_MAX_N);
  if (c->W < 1 || c->H < 1 || c->W > 32767 || c->H > 32767) return failf(-1, "%s: 1 <= W, H <= 32767", who);
  if (c->grid_tile != 0 && c->grid_tile != 16) return failf(-1, "%s: grid_tile must be 0 or 16", who);
  if (!(c->scale > 0.0) || !(c->W_px > 0.0 && c->W_px <= 1e9) || !(c->H_px > 0.0 && c->H_px <= 1e9))
    return failf(-1, "%s: scale > 0, 0 < W_px, H_px <= 1e9", who);
  if (!c->drone || !c->target || !c->dmap) return failf(-1, "%s: a state pointer is NULL", who);
  if (c->N > 0 && (!c->active || !c->kf || !c->trk_radius || !c->trk_prev)) return failf(-1, "%s: a tracker pointer is NULL", who);
  if (!c->th_tab || !c->tt_tab || !c->tie_perm || !c->tie_eq) return failf(-1, "%s: a table pointer is NULL", who);
  if (!c->plan_ok || !c->wp_valid || !c->wp || !c->choice || !c->stat) return failf(-1, "%s: an output pointer is NULL", who);
  return 0;
}

size_t trk_lds(const d2d_jerk_call *c) { return sizeof(double) * 5 * (size_t)(c->N > 0 ? c->N : 1); }

}  // namespace

extern "C" {

int d2d_jerk_version(void) { return D2D_JERK_VERSION; }
const char *d2d_jerk_last_error(void) { return g_err; }

int d2d_jerk_plan(const d2d_jerk_call *c, void *stream) {
  if (const int rc = check_call("d2d_jerk_plan", c)) return rc;
  hipLaunchKernelGGL(jerk_plan_kernel, dim3((unsigned)c->B), dim3(WAVE), trk_lds(c), (hipStream_t)stream, *c);
  return launched("d2d_jerk_plan");
}

int d2d_jerk_plan_live(const d2d_jerk_call *c, const uint8_t *flags, void *stream) {
  if (!flags) return fail(-1, "d2d_jerk_plan_live: flags is NULL (d2d_jerk_plan is the launch without a mask)");
  if (const int rc = check_call("d2d_jerk_plan_live", c)) return rc;
  hipLaunchKernelGGL(jerk_plan_live_kernel, dim3((unsigned)c->B), dim3(WAVE), trk_lds(c), (hipStream_t)stream, *c, flags);
  return launched("d2d_jerk_plan_live");
}

int d2d_jerk_reset(double *trk_radius, uint8_t *trk_prev, const double *trk_radius0, const uint8_t *mask, int32_t mask_stride, int32_t B,
                   int32_t N, void *stream) {
  if (B < 1 || N < 0 || mask_stride < 1) return fail(-1, "d2d_jerk_reset: B >= 1, N >= 0, mask_stride >= 1");
  if (N > D2D_JERK_MAX_N) return failf(-4, "d2d_jerk_reset: N = %d trackers, at most %d", N, D2D_JERK_MAX_N);
  if (N == 0) return 0;
  if (!trk_radius || !trk_prev || !trk_radius0) return fail(-1, "d2d_jerk_reset: a pointer is NULL");
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(jerk_reset_kernel, dim3((unsigned)((total + EW_BLOCK - 1) / EW_BLOCK)), dim3(EW_BLOCK), 0, (hipStream_t)stream,
                     trk_radius, trk_prev, trk_radius0, mask, (int)mask_stride, (int)N, total);
  return launched("d2d_jerk_reset");
}

}  // extern "C"
