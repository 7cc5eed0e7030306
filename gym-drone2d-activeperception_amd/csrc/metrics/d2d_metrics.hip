// d2d_metrics.hip — the difficulty metrics on the device (gfx950): kernels + the C entry points of include/d2d_metrics.h.  Its own
// library (libd2d_metrics.so): it shares no kernel with the step, the closed loop or the worlds.
//
// The velocity-obstacle feasibility metric:
//   geometry    thread = (world, position, agent): arg and theta_ba, coalesced; a second small kernel, thread = (world, position),
//               ORs the collision test over the agents.
//   cones       thread = (world, position, agent): two sin, two cos, two atan2.  d2d_vo_cones reads the half angle, d2d_vo_cones_arg
//               takes it first (d2d_asin.h: up to 15 table doubles of one row, or a seed and a division).  The asin tables stay in
//               global memory (__device__ const, 21 KB): a lane gathers one row of at most 120 B, neighbouring agents' rows differ,
//               and 256 threads would have to copy all 21 KB to LDS to read 256 rows of it; the whole table stays in L2.
//   count       one wave per (world, 64 candidates, 64 positions); lane = candidate.  theta_dif of the wave's candidates against a
//               tile of VO_TILE agents goes to LDS once ([tile][64] doubles), then the wave walks its positions: the cone pairs of
//               (position, tile) arrive with one coalesced load (lane 2a = right, 2a + 1 = left of agent a) and reach every lane
//               through readlane, the lanes test in_between against their LDS column, and the agent loop ends when no lane is
//               still suitable.  Between the tiles lane l keeps the ballot of position l's still-suitable candidates, so N is not
//               capped.  A setup kernel writes 0 / -1 to every count first; the waves add their popcounts (integer atomics: the
//               order cannot change the sum).
//
//
// Traversability:
//   trav_steps  one workgroup per world; the grid is staged in LDS when it has at most TRAV_LDS cells and read from global memory
//               otherwise; thread = (start, direction), in as many passes as 8 * S needs.  Integers only.
//
// Survival fit:
//   fit_first_hit  one wave per (world, 64 positions).  Lane = agent for the updates: the state of up to four tiles of 64 agents
//               stays in registers over all steps.  Lane = position for the tests: position, radius sum of one agent at a time reach
//               every lane through readlane.  No LDS, no barrier, no atomics; the waves of a world's further position tiles repeat
//               the (cheap) agent updates, the first one writes agents_out.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_vo.h, d2d_difficulty.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_VO_QUAL __device__ __forceinline__
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#define D2D_ATAN2_QUAL __device__ __forceinline__
#define D2D_ATAN2_TBL_QUAL __device__ const
#define D2D_ASIN_QUAL __device__ __forceinline__
#define D2D_ASIN_TBL_QUAL __device__ const
#include "d2d_vo.h"
#define D2D_DF_QUAL __device__ __forceinline__
#include "d2d_difficulty.h"

#define WAVE 64
#define VO_TILE 32   /* agents per LDS tile of theta_dif: 32 * 64 * 8 B = 16 KB; 2 * VO_TILE cone doubles = one per lane */
#define VO_PCH 64    /* positions per wave: lane l keeps position l's mask between the tiles */
#define EW_BLOCK 256
#define TRAV_BLOCK 256
#define TRAV_LDS 16384 /* cells of a grid that is staged in LDS (16 KB: 128 x 128); a larger one is read from global memory */
#define FIT_TILES (D2D_FIT_MAX_N / WAVE)

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
  const double *ag = agents + (size_t)(bp / P) * D2D_AF * N;
  double a, t;
  d2d_vo_pair(pos[2 * p], pos[2 * p + 1], ag[D2D_A_PX * N + j], ag[D2D_A_PY * N + j], rA, ag[D2D_A_R * N + j], &a, &t);
  arg[i] = a;
  theta_ba[i] = t;
}

__global__ __launch_bounds__(EW_BLOCK) void vo_collided_kernel(const double *__restrict__ agents, const double *__restrict__ pos, double rA,
                                                              int N, int P, long long BP, uint8_t *__restrict__ collided) {
  const long long bp = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (bp >= BP) return;
  const int p = (int)(bp % P);
  const double *ag = agents + (size_t)(bp / P) * D2D_AF * N;
  const double ax = pos[2 * p], ay = pos[2 * p + 1];
  int hit = 0;
  for (int j = 0; j < N; ++j) hit |= d2d_vo_hits(ax, ay, ag[D2D_A_PX * N + j], ag[D2D_A_PY * N + j], rA, ag[D2D_A_R * N + j]);
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

template <bool HALF_OUT>
__global__ __launch_bounds__(EW_BLOCK) void vo_cones_arg_kernel(const double *__restrict__ theta_ba, const double *__restrict__ arg,
                                                               const uint8_t *__restrict__ collided, int N, long long total,
                                                               double *__restrict__ half_out, double *__restrict__ cone) {
  const long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (i >= total) return;
  const bool hit = collided[i / N];
  double r = 0.0, l = 0.0;
  if (HALF_OUT || !hit) {                       // (a collided position's half angles are only ever read through half_out)
    const double half = d2d_vo_half(arg[i]);
    if (HALF_OUT) half_out[i] = half;
    if (!hit) d2d_vo_cone(theta_ba[i], half, &r, &l);
  }
  cone[2 * i] = r;
  cone[2 * i + 1] = l;
}

__global__ __launch_bounds__(EW_BLOCK) void asin_array_kernel(const double *x, long long n, double *out) {   // out may alias x
  const long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (i < n) out[i] = d2d_asin(x[i]);
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
  const double *ag = agents + (size_t)b * D2D_AF * N;
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
      td[a * WAVE + lane] = valid ? d2d_vo_theta_dif(cx, cy, ag[D2D_A_VX * N + a0 + a], ag[D2D_A_VY * N + a0 + a]) : 0.0;
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

template <bool STAGED>
__global__ __launch_bounds__(TRAV_BLOCK) void trav_steps_kernel(const uint8_t *__restrict__ gt, int W, int H, const int32_t *__restrict__ starts,
                                                               int S, int32_t *__restrict__ steps) {
  __shared__ uint8_t cells[STAGED ? TRAV_LDS : 4];
  const uint8_t *g = gt + (size_t)blockIdx.x * W * H;
  if constexpr (STAGED) {
    const int n = W * H;                        // <= TRAV_LDS
    for (int c = threadIdx.x; c < n; c += TRAV_BLOCK) cells[c] = g[c];
    __syncthreads();
  }
  const uint8_t *grid = STAGED ? cells : g;
  int32_t *out = steps + (size_t)blockIdx.x * S * 8;
  for (int t = threadIdx.x; t < 8 * S; t += TRAV_BLOCK) {
    const int i = starts[2 * (t >> 3)], j = starts[2 * (t >> 3) + 1];
    out[t] = d2d_trav_open(grid, W, H, i, j) ? d2d_trav_ray(grid, W, H, i, j, t & 7) : -1;
  }
}

template <int NT>   // tiles of 64 agents: 64 * (NT - 1) < N <= 64 * NT
__global__ __launch_bounds__(WAVE) void fit_first_hit_kernel(const double *__restrict__ agents, const double *__restrict__ pos, double drone_radius,
                                                            double W_px, double H_px, double scale, double dt, int N, int P, int checks,
                                                            int32_t *__restrict__ first, double *__restrict__ agents_out) {
  const int lane = threadIdx.x;
  const long long p = (long long)blockIdx.y * WAVE + lane;
  const double *ag = agents + (size_t)blockIdx.x * D2D_AF * N;
  double px[NT], py[NT], vx[NT], vy[NT], r[NT], rr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = t * WAVE + lane;
    const bool live = j < N;                    // lanes beyond N neither load nor store
    px[t] = live ? ag[D2D_A_PX * N + j] : 0.0;
    py[t] = live ? ag[D2D_A_PY * N + j] : 0.0;
    vx[t] = live ? ag[D2D_A_VX * N + j] : 0.0;
    vy[t] = live ? ag[D2D_A_VY * N + j] : 0.0;
    r[t] = live ? ag[D2D_A_R * N + j] : 0.0;
    rr[t] = r[t] + drone_radius;
  }
  const bool mine = p < P;                      // lanes beyond P neither load nor store
  const double ax = mine ? pos[2 * p] : 0.0, ay = mine ? pos[2 * p + 1] : 0.0;
  int32_t f = -1;
  for (int k = -1; k < checks; ++k) {
    if (k >= 0 && __ballot(mine && f < 0) != 0ull) {   // (a tile whose positions have all been hit only moves the agents on)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int na = min(WAVE, N - t * WAVE);
        for (int a = 0; a < na; ++a) {
          const double bx = readlane_f64(px[t], a), by = readlane_f64(py[t], a), brr = readlane_f64(rr[t], a);
          if (f < 0 && d2d_fit_hits(ax, ay, bx, by, brr)) f = k;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t * WAVE + lane < N) d2d_fit_agent_step(&px[t], &py[t], &vx[t], &vy[t], r[t], W_px, H_px, scale, dt);
  }
  if (mine) first[(size_t)blockIdx.x * P + p] = f;
  if (agents_out != nullptr && blockIdx.y == 0) {
    double *o = agents_out + (size_t)blockIdx.x * D2D_AF * N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int j = t * WAVE + lane;
      if (j < N) {
        o[D2D_A_PX * N + j] = px[t];
        o[D2D_A_PY * N + j] = py[t];
        o[D2D_A_VX * N + j] = vx[t];
        o[D2D_A_VY * N + j] = vy[t];
        o[D2D_A_R * N + j] = r[t];
        o[D2D_A_R2 * N + j] = ag[D2D_A_R2 * N + j];
      }
    }
  }
}

int check_sizes(const char *who, long long B, long long N, long long P, long long C) {
  if (B < 1 || N < 1 || P < 1 || C < 1) return failf(-1, "%s: B, N, P, C >= 1", who);
  if (B > D2D_VO_MAX_B || P > D2D_VO_MAX_P || B * P > D2D_VO_MAX_ELEMS / (2 * N))
    return failf(-4, "%s: B <= %d, P <= %d and B * P * N * 2 <= %d", who, D2D_VO_MAX_B, D2D_VO_MAX_P, D2D_VO_MAX_ELEMS);
  return 0;
}

int launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  return failf(-3, "%s: launch failed: %s", who, hipGetErrorString(err));
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

int d2d_vo_cones_arg(const double *theta_ba, const double *arg, const uint8_t *collided, int32_t B, int32_t N, int32_t P,
                     double *half_out, double *cone, void *stream) {
  if (const int rc = check_sizes("d2d_vo_cones_arg", B, N, P, 1)) return rc;
  if (!theta_ba || !arg || !collided || !cone) return fail(-1, "d2d_vo_cones_arg: a pointer is NULL");
  const long long total = (long long)B * P * N;
  if (half_out)
    hipLaunchKernelGGL(vo_cones_arg_kernel<true>, dim3(blocks_of(total)), dim3(EW_BLOCK), 0, (hipStream_t)stream, theta_ba, arg, collided,
                       (int)N, total, half_out, cone);
  else
    hipLaunchKernelGGL(vo_cones_arg_kernel<false>, dim3(blocks_of(total)), dim3(EW_BLOCK), 0, (hipStream_t)stream, theta_ba, arg, collided,
                       (int)N, total, half_out, cone);
  return launched("d2d_vo_cones_arg");
}

int d2d_asin_array(const double *x, int64_t n, double *out, void *stream) {
  if (n < 0 || !x || !out) return fail(-1, "d2d_asin_array: n >= 0 and no NULL pointer");
  if (n > (int64_t)D2D_VO_MAX_ELEMS * EW_BLOCK) return fail(-4, "d2d_asin_array: n <= (2^31 - 1) * 256");
  if (n == 0) return 0;
  hipLaunchKernelGGL(asin_array_kernel, dim3(blocks_of(n)), dim3(EW_BLOCK), 0, (hipStream_t)stream, x, (long long)n, out);
  return launched("d2d_asin_array");
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

int d2d_trav_steps(const uint8_t *gt, int32_t B, int32_t W, int32_t H, const int32_t *starts, int32_t S, int32_t *steps, void *stream) {
  if (B < 1 || W < 1 || H < 1 || S < 1) return fail(-1, "d2d_trav_steps: B, W, H, S >= 1");
  if (!gt || !starts || !steps) return fail(-1, "d2d_trav_steps: a pointer is NULL");
  if ((long long)W * H > D2D_TRAV_MAX_ELEMS || (long long)B * S * 8 > D2D_TRAV_MAX_ELEMS)
    return fail(-4, "d2d_trav_steps: W * H <= 2^31 - 1 and B * S * 8 <= 2^31 - 1");
  if ((long long)W * H <= TRAV_LDS)
    hipLaunchKernelGGL(trav_steps_kernel<true>, dim3((unsigned)B), dim3(TRAV_BLOCK), 0, (hipStream_t)stream, gt, (int)W, (int)H, starts, (int)S,
                       steps);
  else
    hipLaunchKernelGGL(trav_steps_kernel<false>, dim3((unsigned)B), dim3(TRAV_BLOCK), 0, (hipStream_t)stream, gt, (int)W, (int)H, starts, (int)S,
                       steps);
  return launched("d2d_trav_steps");
}

int d2d_fit_first_hit(const double *agents, const double *pos, double drone_radius, double W_px, double H_px, double scale, double dt,
                      int32_t B, int32_t N, int32_t P, int32_t checks, int32_t *first, double *agents_out, void *stream) {
  if (B < 1 || N < 1 || P < 1 || checks < 0) return fail(-1, "d2d_fit_first_hit: B, N, P >= 1 and checks >= 0");
  if (!agents || !pos || !first) return fail(-1, "d2d_fit_first_hit: a pointer is NULL");
  if (N > D2D_FIT_MAX_N || P > D2D_FIT_MAX_P || (long long)B * P > D2D_FIT_MAX_ELEMS || (long long)B * D2D_AF * N > D2D_FIT_MAX_ELEMS)
    return failf(-4, "d2d_fit_first_hit: N <= %d, P <= %d and B * max(P, 6 * N) <= %d", D2D_FIT_MAX_N, D2D_FIT_MAX_P, D2D_FIT_MAX_ELEMS);
  const dim3 grid((unsigned)B, (unsigned)((P + WAVE - 1) / WAVE));
#define FIT_LAUNCH(NT)                                                                                                                  \
  hipLaunchKernelGGL(fit_first_hit_kernel<NT>, grid, dim3(WAVE), 0, (hipStream_t)stream, agents, pos, drone_radius, W_px, H_px, scale, dt, \
                     (int)N, (int)P, (int)checks, first, agents_out)
  static_assert(FIT_TILES == 4, "one case per tile count");
  switch ((N + WAVE - 1) / WAVE) {
    case 1: FIT_LAUNCH(1); break;
    case 2: FIT_LAUNCH(2); break;
    case 3: FIT_LAUNCH(3); break;
    default: FIT_LAUNCH(4); break;
  }
#undef FIT_LAUNCH
  return launched("d2d_fit_first_hit");
}

}  // extern "C"
