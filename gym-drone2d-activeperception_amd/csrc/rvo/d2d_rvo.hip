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
//   *_live         the same two for a batch with finished envs (include/d2d_rvo_live.h): the bodies are shared, the test of the env's
//                  done flag comes first.  It is uniform over a rvo_velocity wave, which then copies the agent's velocity (lanes 0 and
//                  1, one entry each) and ends before any cone is built.
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
#include "../../../include/d2d_rvo_live.h"

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
#include "d2d_rvo_wave.inc"   // the body, shared as text with rvo_velocity_live_kernel: this kernel compiles to what it always did
}

__global__ __launch_bounds__(WAVE) void rvo_velocity_live_kernel(const double *__restrict__ agents, const double *__restrict__ vel,
                                                                const int32_t *__restrict__ pillars,
                                                                const uint8_t *__restrict__ flags, int N, int P,
                                                                double *__restrict__ vel_out) {
  const size_t env = blockIdx.x / (unsigned)N;
  if (flags[env * 4 + D2D_RVO_LIVE_F_DONE]) {          // one env per wave: no lane goes on
    const size_t at = env * 2 * N + (size_t)threadIdx.x * N + blockIdx.x % (unsigned)N;
    if (threadIdx.x < 2) vel_out[at] = vel[at];
    return;
  }
#include "d2d_rvo_wave.inc"
}

__device__ __forceinline__ void rvo_agent_step_of(double *agents, const double *vel, double W_px, double H_px, double scale, double dt, int N,
                                                  size_t b, int i) {
  double *ag = agents + b * D2D_AF * N;
  const double *v = vel + b * 2 * N;
  double px = ag[D2D_A_PX * N + i], py = ag[D2D_A_PY * N + i], fx = ag[D2D_A_VX * N + i], fy = ag[D2D_A_VY * N + i];
  d2d_rvo_agent_step(&px, &py, &fx, &fy, v[i], v[N + i], ag[D2D_A_R * N + i], W_px, H_px, scale, dt);
  ag[D2D_A_PX * N + i] = px;
  ag[D2D_A_PY * N + i] = py;
  ag[D2D_A_VX * N + i] = fx;
  ag[D2D_A_VY * N + i] = fy;
}

__global__ __launch_bounds__(EW_BLOCK) void rvo_agents_step_kernel(double *__restrict__ agents, const double *__restrict__ vel, double W_px,
                                                                  double H_px, double scale, double dt, int N, long long total) {
  const long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (t >= total) return;
  rvo_agent_step_of(agents, vel, W_px, H_px, scale, dt, N, (size_t)(t / N), (int)(t % N));
}

__global__ __launch_bounds__(EW_BLOCK) void rvo_agents_step_live_kernel(double *__restrict__ agents, const double *__restrict__ vel,
                                                                       const uint8_t *__restrict__ flags, double W_px, double H_px,
                                                                       double scale, double dt, int N, long long total) {
  const long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (t >= total) return;
  const size_t b = (size_t)(t / N);
  if (flags[b * 4 + D2D_RVO_LIVE_F_DONE]) return;
  rvo_agent_step_of(agents, vel, W_px, H_px, scale, dt, N, b, (int)(t % N));
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

int d2d_rvo_velocity_live(const double *agents, const double *vel, const int32_t *pillars, const uint8_t *flags, int32_t B, int32_t N,
                          int32_t P, double *vel_out, void *stream) {
  if (const int rc = check_sizes("d2d_rvo_velocity_live", B, N, P)) return rc;
  if (!flags) return fail(-1, "d2d_rvo_velocity_live: flags is NULL (d2d_rvo_velocity is the launch without a mask)");
  if (N == 0) return 0;
  if (!agents || !vel || !vel_out || (P > 0 && !pillars)) return fail(-1, "d2d_rvo_velocity_live: a pointer is NULL");
  if (vel_out == vel) return fail(-1, "d2d_rvo_velocity_live: vel_out must not be vel");
  const size_t lds = sizeof(double) * D2D_RVO_CONE_F * (size_t)(N - 1 + P);
  hipLaunchKernelGGL(rvo_velocity_live_kernel, dim3((unsigned)((long long)B * N)), dim3(WAVE), lds, (hipStream_t)stream, agents, vel,
                     pillars, flags, (int)N, (int)P, vel_out);
  return launched("d2d_rvo_velocity_live");
}

int d2d_rvo_agents_step_live(double *agents, const double *vel, const uint8_t *flags, double W_px, double H_px, double scale, double dt,
                             int32_t B, int32_t N, void *stream) {
  if (const int rc = check_sizes("d2d_rvo_agents_step_live", B, N, 0)) return rc;
  if (!flags) return fail(-1, "d2d_rvo_agents_step_live: flags is NULL (d2d_rvo_agents_step is the launch without a mask)");
  if (N == 0) return 0;
  if (!agents || !vel) return fail(-1, "d2d_rvo_agents_step_live: a pointer is NULL");
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(rvo_agents_step_live_kernel, dim3((unsigned)((total + EW_BLOCK - 1) / EW_BLOCK)), dim3(EW_BLOCK), 0,
                     (hipStream_t)stream, agents, vel, flags, W_px, H_px, scale, dt, (int)N, total);
  return launched("d2d_rvo_agents_step_live");
}

}  // extern "C"
