// d2d_metrics.hip — the velocity-obstacle feasibility metric on the device (gfx950): kernels + the C entry points of
// include/d2d_metrics.h.  Its own library (libd2d_metrics.so): it shares no kernel with the step, the closed loop or the worlds.
//
//   geometry    thread = (world, position, agent): arg and theta_ba, coalesced; a second small kernel, thread = (world, position),
//               ORs the collision test over the agents.
//   cones       thread = (world, position, agent): two sin, two cos, two atan2.
//   count       one wave per (world, 64 candidates, 64 positions); lane = candidate.  theta_dif of the wave's candidates against a
//               tile of VO_TILE agents goes to LDS once ([tile][64] doubles), then the wave walks its positions: the cone pairs of
//               (position, tile) arrive with one coalesced load (lane 2a = right, 2a + 1 = left of agent a) and reach every lane
//               through readlane, the lanes test in_between against their LDS column, and the agent loop ends when no lane is
//               still suitable.  Between the tiles lane l keeps the ballot of position l's still-suitable candidates, so N is not
//               capped.  A setup kernel writes 0 / -1 to every count first; the waves add their popcounts (integer atomics: the
//               order cannot change the sum).
//
// Arithmetic is fp64 in the reference's own operation order (d2d_vo.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_VO_QUAL __device__ __forceinline__
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#define D2D_ATAN2_QUAL __device__ __forceinline__
#define D2D_ATAN2_TBL_QUAL __device__ const
#include "d2d_vo.h"

#define WAVE 64
#define VO_TILE 32   /* agents per LDS tile of theta_dif: 32 * 64 * 8 B = 16 KB; 2 * VO_TILE cone doubles = one per lane */
#define VO_PCH 64    /* positions per wave: lane l keeps position l's mask between the tiles */
#define EW_BLOCK 256

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

__device__ __forceinline__ double readlane_f64(double v, int src) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long b, int src) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(EW_BLOCK) void vo_pairs_kernel(const double *__restrict__ agents, const double *__restrict__ pos, double rA,
                                                           int N, int P, long long total, double *__restrict__ arg,
                                                           double *__restrict__ theta_ba) {
  const long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % N);
  const long long bp = i / N;
  const int p = (int)(bp % P);
  const double *ag = agents + (size_t)(bp / P) * D2D_VO_AF * N;
  double a, t;
  d2d_vo_pair(pos[2 * p], pos[2 * p + 1], ag[D2D_VO_A_PX * N + j], ag[D2D_VO_A_PY * N + j], rA, ag[D2D_VO_A_R * N + j], &a, &t);
  arg[i] = a;
  theta_ba[i] = t;
}

__global__ __launch_bounds__(EW_BLOCK) void vo_collided_kernel(const double *__restrict__ agents, const double *__restrict__ pos, double rA,
                                                              int N, int P, long long BP, uint8_t *__restrict__ collided) {
  const long long bp = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (bp >= BP) return;
  const int p = (int)(bp % P);
  const double *ag = agents + (size_t)(bp / P) * D2D_VO_AF * N;
  const double ax = pos[2 * p], ay = pos[2 * p + 1];
  int hit = 0;
  for (int j = 0; j < N; ++j) hit |= d2d_vo_hits(ax, ay, ag[D2D_VO_A_PX * N + j], ag[D2D_VO_A_PY * N + j], rA, ag[D2D_VO_A_R * N + j]);
  collided[bp] = (uint8_t)hit;
}

__global__ __launch_bounds__(EW_BLOCK) void vo_cones_kernel(const double *__restrict__ theta_ba, const double *__restrict__ half,
                                                           const uint8_t *__restrict__ collided, int N, long long total,
                                                           double *__restrict__ cone) {
  const long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (i >= total) return;
  double r = 0.0, l = 0.0;
  if (!collided[i / N]) d2d_vo_cone(theta_ba[i], half[i], &r, &l);
  cone[2 * i] = r;
  cone[2 * i + 1] = l;
}

__global__ __launch_bounds__(EW_BLOCK) void vo_count_init_kernel(const uint8_t *__restrict__ collided, long long BP, int32_t *__restrict__ count) {
  const long long bp = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (bp < BP) count[bp] = collided[bp] ? -1 : 0;
}

__global__ __launch_bounds__(WAVE) void vo_count_kernel(const double *__restrict__ agents, const double *__restrict__ cand,
                                                       const double *__restrict__ cone, const uint8_t *__restrict__ collided, int N, int P,
                                                       int C, int32_t *__restrict__ count) {
  __shared__ double td[VO_TILE * WAVE];
  const int lane = threadIdx.x;
  const long long c = (long long)blockIdx.x * WAVE + lane;
  const int p0 = blockIdx.y * VO_PCH, b = blockIdx.z;
  const int np = min(VO_PCH, P - p0);
  const size_t bp0 = (size_t)b * P + p0;
  const double *ag = agents + (size_t)b * D2D_VO_AF * N;
  const bool valid = c < C;
  const double cx = valid ? cand[2 * c] : 0.0, cy = valid ? cand[2 * c + 1] : 0.0;
  const unsigned long long vm = __ballot(valid);
  const bool mine = lane < np && !collided[bp0 + (lane < np ? lane : 0)];
  unsigned long long mask = mine ? vm : 0ull;   // lane l: the candidates of this wave still suitable at position p0 + l
  if (__ballot(mask != 0ull) == 0ull) return;   // every position of the chunk is collided

  for (int a0 = 0; a0 < N; a0 += VO_TILE) {
    const int na = min(VO_TILE, N - a0);
    __syncthreads();                            // the previous tile has been read
    for (int a = 0; a < na; ++a)
      td[a * WAVE + lane] = valid ? d2d_vo_theta_dif(cx, cy, ag[D2D_VO_A_VX * N + a0 + a], ag[D2D_VO_A_VY * N + a0 + a]) : 0.0;
    __syncthreads();
    for (int pi = 0; pi < np; ++pi) {
      const unsigned long long m = readlane_u64(mask, pi);
      if (m == 0ull) continue;                  // collided, or no candidate of this wave left
      const double cv = lane < 2 * na ? cone[((bp0 + pi) * N + a0) * 2 + lane] : 0.0;
      bool suit = (m >> lane) & 1ull;
      for (int a = 0; a < na; ++a) {
        const double right = readlane_f64(cv, 2 * a), left = readlane_f64(cv, 2 * a + 1);
        if (suit && d2d_vo_in_between(right, td[a * WAVE + lane], left)) suit = false;
        if (__ballot(suit) == 0ull) break;
      }
      const unsigned long long nm = __ballot(suit);
      if (lane == pi) mask = nm;
    }
  }
  if (mine) atomicAdd(count + bp0 + lane, (int32_t)__popcll(mask));
}

int check_sizes(const char *who, long long B, long long N, long long P, long long C) {
  char msg[200];
  if (B < 1 || N < 1 || P < 1 || C < 1) {
    snprintf(msg, sizeof msg, "%s: B, N, P, C >= 1", who);
    return fail(-1, msg);
  }
  if (B > D2D_VO_MAX_B || P > D2D_VO_MAX_P || B * P > D2D_VO_MAX_ELEMS / (2 * N)) {
    snprintf(msg, sizeof msg, "%s: B <= %d, P <= %d and B * P * N * 2 <= %d", who, D2D_VO_MAX_B, D2D_VO_MAX_P, D2D_VO_MAX_ELEMS);
    return fail(-4, msg);
  }
  return 0;
}

int launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "%s: launch failed: %s", who, hipGetErrorString(err));
  return -3;
}

unsigned blocks_of(long long n) { return (unsigned)((n + EW_BLOCK - 1) / EW_BLOCK); }

}  // namespace

extern "C" {

int d2d_metrics_version(void) { return D2D_METRICS_VERSION; }
const char *d2d_metrics_last_error(void) { return g_err; }

int d2d_vo_geometry(const double *agents, const double *pos, double rA, int32_t B, int32_t N, int32_t P, double *arg, double *theta_ba,
                    uint8_t *collided, void *stream) {
  if (const int rc = check_sizes("d2d_vo_geometry", B, N, P, 1)) return rc;
  if (!agents || !pos || !arg || !theta_ba || !collided) return fail(-1, "d2d_vo_geometry: a pointer is NULL");
  const long long BP = (long long)B * P, total = BP * N;
  hipLaunchKernelGGL(vo_pairs_kernel, dim3(blocks_of(total)), dim3(EW_BLOCK), 0, (hipStream_t)stream, agents, pos, rA, (int)N, (int)P,
                     total, arg, theta_ba);
  if (const int rc = launched("d2d_vo_geometry")) return rc;
  hipLaunchKernelGGL(vo_collided_kernel, dim3(blocks_of(BP)), dim3(EW_BLOCK), 0, (hipStream_t)stream, agents, pos, rA, (int)N, (int)P, BP,
                     collided);
  return launched("d2d_vo_geometry");
}

int d2d_vo_cones(const double *theta_ba, const double *half, const uint8_t *collided, int32_t B, int32_t N, int32_t P, double *cone,
                 void *stream) {
  if (const int rc = check_sizes("d2d_vo_cones", B, N, P, 1)) return rc;
  if (!theta_ba || !half || !collided || !cone) return fail(-1, "d2d_vo_cones: a pointer is NULL");
  const long long total = (long long)B * P * N;
  hipLaunchKernelGGL(vo_cones_kernel, dim3(blocks_of(total)), dim3(EW_BLOCK), 0, (hipStream_t)stream, theta_ba, half, collided, (int)N,
                     total, cone);
  return launched("d2d_vo_cones");
}

int d2d_vo_count(const double *agents, const double *cand, const double *cone, const uint8_t *collided, int32_t B, int32_t N, int32_t P,
                 int32_t C, int32_t *count, void *stream) {
  if (const int rc = check_sizes("d2d_vo_count", B, N, P, C)) return rc;
  if (!agents || !cand || !cone || !collided || !count) return fail(-1, "d2d_vo_count: a pointer is NULL");
  const long long BP = (long long)B * P;
  hipLaunchKernelGGL(vo_count_init_kernel, dim3(blocks_of(BP)), dim3(EW_BLOCK), 0, (hipStream_t)stream, collided, BP, count);
  if (const int rc = launched("d2d_vo_count")) return rc;
  const dim3 grid((unsigned)(((long long)C + WAVE - 1) / WAVE), (unsigned)((P + VO_PCH - 1) / VO_PCH), (unsigned)B);
  hipLaunchKernelGGL(vo_count_kernel, grid, dim3(WAVE), 0, (hipStream_t)stream, agents, cand, cone, collided, (int)N, (int)P, (int)C, count);
  return launched("d2d_vo_count");
}

}  // extern "C"
