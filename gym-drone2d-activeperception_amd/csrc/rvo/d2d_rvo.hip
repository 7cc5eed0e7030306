// d2d_rvo.hip — the RVO motion profile on the device (gfx950): kernels + the C entry points of include/d2d_rvo.h.  Its own library
// (libd2d_rvo.so): it shares no kernel with the step, the closed loop, the worlds or the metrics.
//
//   rvo_velocity   one wave per (env, agent).
//                  cones       lane = cone: the N - 1 + P cones of this agent go to LDS as six planes of doubles ([6][cones], so that
//                              lane k's writes fall on consecutive banks); per cone two atan2 of (sin, cos), one asin, one norm.
//                  candidates  lane = candidate, 64 at a time (161 = 2 * 64 + 33, 193 = 3 * 64 + 1).  Every lane reads the same cone
//                              at the same time (an LDS broadcast) and takes one atan2 per (candidate, cone); the cone loop ends
//                              when no lane is still suitable.  A lane keeps the best (key, index) of its own candidates, which it
//                              meets in rising index order.
//                  no candidate suitable (rare: 3 of 480 decisions in the recorded pillar world): a second walk over the cones
//                              that takes the time-to-collision term wherever in_between holds, in cone order, as Python's min
//                              meets them.
//                  reduction   (key, index) over the wave by xor shuffles: smaller key, then lower index.  NaN keys never enter it;
//                              a NaN key of candidate 0 is turned into -inf first, since Python's min returns the first element
//                              when that is a NaN and no key is negative.  (No finite input produces a NaN key: include/d2d_rvo.h.)
//                  The winner's two doubles are recomputed from its index and written by lane 0.
//   rvo_agents_step  thread = (env, agent): Agent.step, coalesced over the agents' planes.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_rvo.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_RVO_QUAL __device__ __forceinline__
#define D2D_RVO_TBL_QUAL __device__ const
#define D2D_VO_QUAL __device__ __forceinline__
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#define D2D_ATAN2_QUAL __device__ __forceinline__
#define D2D_ATAN2_TBL_QUAL __device__ const
#define D2D_ASIN_QUAL __device__ __forceinline__
#define D2D_ASIN_TBL_QUAL __device__ const
#include "d2d_rvo.h"

#define WAVE 64
#define EW_BLOCK 256
#define NO_INDEX 0x7fffffff

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

__global__ __launch_bounds__(WAVE) void rvo_velocity_kernel(const double *__restrict__ agents, const double *__restrict__ vel,
                                                           const int32_t *__restrict__ pillars, int N, int P,
                                                           double *__restrict__ vel_out) {
  extern __shared__ __attribute__((aligned(16))) double cones[];   // [6][nc]
  const int lane = threadIdx.x;
  const int i = (int)(blockIdx.x % (unsigned)N);
  const size_t b = blockIdx.x / (unsigned)N;
  const int nc = N - 1 + P;
  const double *ag = agents + b * D2D_AF * N, *v = vel + b * 2 * N;
  const int32_t *pil = pillars + b * P * 3;                          // (not read when P == 0)
  const double rob_rad = ag[D2D_A_R * N] + 0.01;
  const double pax = ag[D2D_A_PX * N + i], pay = ag[D2D_A_PY * N + i];
  const double prefx = ag[D2D_A_VX * N + i], prefy = ag[D2D_A_VY * N + i];

  for (int k = lane; k < nc; k += WAVE) d2d_rvo_cone_of(ag, v, pil, N, i, k, rob_rad, cones + k, (size_t)nc);
  __syncthreads();
  const double *apx = cones, *apy = cones + nc, *right = cones + 2 * nc, *left = cones + 3 * nc, *dist = cones + 4 * nc,
               *rad = cones + 5 * nc;

  double delta;
  const int nrad = d2d_rvo_radii(d2d_vo_norm(prefx, prefy), &delta);
  const int C = D2D_RVO_NTHETA * nrad + 1;

  double best_key = INFINITY;
  int best = NO_INDEX;
  for (int c0 = 0; c0 < C; c0 += WAVE) {            // min(suitable_V, key=norm(v - pref))
    const int c = c0 + lane;
    double cx, cy, td, dx, dy;
    d2d_rvo_candidate(c < C ? c : C - 1, nrad, delta, prefx, prefy, &cx, &cy);
    bool suit = c < C;
    for (int k = 0; k < nc; ++k) {
      if (__ballot(suit) == 0ull) break;
      if (suit && d2d_rvo_inside(cx, cy, pax, pay, apx[k], apy[k], right[k], left[k], &td, &dx, &dy)) suit = false;
    }
    if (suit) {
      const double key = d2d_vo_norm(cx - prefx, cy - prefy);
      if (key < best_key) best_key = key, best = c;  // (never a NaN, never +inf: the first candidate of the lane always enters)
    }
  }
  if (__ballot(best != NO_INDEX) == 0ull) {          // min(unsuitable_V, key=0.2 / tc_V + norm(v - pref)): every candidate
    for (int c0 = 0; c0 < C; c0 += WAVE) {
      const int c = c0 + lane;
      if (c >= C) continue;
      double cx, cy, td, dx, dy, tc = 0.0;
      bool have = false;
      d2d_rvo_candidate(c, nrad, delta, prefx, prefy, &cx, &cy);
      for (int k = 0; k < nc; ++k)
        if (d2d_rvo_inside(cx, cy, pax, pay, apx[k], apy[k], right[k], left[k], &td, &dx, &dy)) {
          const double t = d2d_rvo_tc(td, dx, dy, right[k], left[k], dist[k], rad[k]);
          if (!have || t < tc) tc = t;
          have = true;
        }
      double key = d2d_rvo_key(tc, cx, cy, prefx, prefy);
      if (key != key) {
        if (c != 0) continue;                        // a NaN that is not the list's first element never wins
        key = -INFINITY;                             // the first element does, whatever follows (every other key is >= 0)
      }
      if (key < best_key || (key == best_key && c < best)) best_key = key, best = c;
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m > 0; m >>= 1) {
    const double ok = __shfl_xor(best_key, m, WAVE);
    const int oi = __shfl_xor(best, m, WAVE);
    if (ok < best_key || (ok == best_key && oi < best)) best_key = ok, best = oi;
  }
  if (lane == 0) {
    double cx, cy;
    d2d_rvo_candidate(best, nrad, delta, prefx, prefy, &cx, &cy);
    double *out = vel_out + b * 2 * N;
    out[i] = cx;
    out[N + i] = cy;
  }
}

__global__ __launch_bounds__(EW_BLOCK) void rvo_agents_step_kernel(double *__restrict__ agents, const double *__restrict__ vel, double W_px,
                                                                  double H_px, double scale, double dt, int N, long long total) {
  const long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (t >= total) return;
  const int i = (int)(t % N);
  const size_t b = (size_t)(t / N);
  double *ag = agents + b * D2D_AF * N;
  const double *v = vel + b * 2 * N;
  double px = ag[D2D_A_PX * N + i], py = ag[D2D_A_PY * N + i], fx = ag[D2D_A_VX * N + i], fy = ag[D2D_A_VY * N + i];
  d2d_rvo_agent_step(&px, &py, &fx, &fy, v[i], v[N + i], ag[D2D_A_R * N + i], W_px, H_px, scale, dt);
  ag[D2D_A_PX * N + i] = px;
  ag[D2D_A_PY * N + i] = py;
  ag[D2D_A_VX * N + i] = fx;
  ag[D2D_A_VY * N + i] = fy;
}

int check_sizes(const char *who, long long B, long long N, long long P) {
  if (B < 1 || N < 0 || P < 0) return failf(-1, "%s: B >= 1, N >= 0, P >= 0", who);
  if (N > 0 && N - 1 + P > D2D_RVO_MAX_CONES)
    return failf(-4, "%s: N - 1 + P = %lld cones, at most %d fit the wave's LDS", who, N - 1 + P, D2D_RVO_MAX_CONES);
  if (N > 0 && B > D2D_RVO_MAX_ELEMS / (D2D_AF * N)) return failf(-4, "%s: B * 6 * N <= %d", who, D2D_RVO_MAX_ELEMS);
  return 0;
}

int launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  return failf(-3, "%s: launch failed: %s", who, hipGetErrorString(err));
}

}  // namespace

extern "C" {

int d2d_rvo_version(void) { return D2D_RVO_VERSION; }
const char *d2d_rvo_last_error(void) { return g_err; }

int d2d_rvo_velocity(const double *agents, const double *vel, const int32_t *pillars, int32_t B, int32_t N, int32_t P, double *vel_out,
                     void *stream) {
  if (const int rc = check_sizes("d2d_rvo_velocity", B, N, P)) return rc;
  if (N == 0) return 0;
  if (!agents || !vel || !vel_out || (P > 0 && !pillars)) return fail(-1, "d2d_rvo_velocity: a pointer is NULL");
  if (vel_out == vel) return fail(-1, "d2d_rvo_velocity: vel_out must not be vel");
  const size_t lds = sizeof(double) * D2D_RVO_CONE_F * (size_t)(N - 1 + P);
  hipLaunchKernelGGL(rvo_velocity_kernel, dim3((unsigned)((long long)B * N)), dim3(WAVE), lds, (hipStream_t)stream, agents, vel, pillars,
                     (int)N, (int)P, vel_out);
  return launched("d2d_rvo_velocity");
}

int d2d_rvo_agents_step(double *agents, const double *vel, double W_px, double H_px, double scale, double dt, int32_t B, int32_t N,
                        void *stream) {
  if (const int rc = check_sizes("d2d_rvo_agents_step", B, N, 0)) return rc;
  if (N == 0) return 0;
  if (!agents || !vel) return fail(-1, "d2d_rvo_agents_step: a pointer is NULL");
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(rvo_agents_step_kernel, dim3((unsigned)((total + EW_BLOCK - 1) / EW_BLOCK)), dim3(EW_BLOCK), 0, (hipStream_t)stream,
                     agents, vel, W_px, H_px, scale, dt, (int)N, total);
  return launched("d2d_rvo_agents_step");
}

}  // extern "C"
