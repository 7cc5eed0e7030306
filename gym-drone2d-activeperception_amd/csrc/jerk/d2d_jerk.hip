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
  extern __shared__ __attribute__((aligned(16))) double trk[];   // [5][cap]
  __shared__ double cost[NT];
  __shared__ int order[NT];
  __shared__ int seen[NT];
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  const int N = c.N, cap = N > 0 ? N : 1, S = c.S;

  // ---- trackers: archive bookkeeping (utils.py:184, 238) and the active ones into LDS ----
  int na = 0;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    bool act = false;
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, rad = 0;
    if (k < N) {
      const size_t ik = b * N + k;
      const double *mu = c.kf + ik * D2D_JERK_KF;
      m0 = mu[0]; m1 = mu[1]; m2 = mu[2]; m3 = mu[3];
      act = c.active[ik] != 0;
      const bool prev = c.trk_prev[ik] != 0;
      rad = c.trk_radius[ik];
      if (prev && !act) {
        rad = c.agent_radius;
        c.trk_radius[ik] = rad;
      }
      if (prev != act) c.trk_prev[ik] = act ? 1 : 0;
    }
    const unsigned long long am = __ballot(act);
    if (act) {
      const int q = na + __popcll(am & ((1ull << lane) - 1ull));   // q < N <= cap
      trk[q] = m0; trk[cap + q] = m1; trk[2 * cap + q] = m2; trk[3 * cap + q] = m3;
      trk[4 * cap + q] = c.drone_radius + rad + 5.0 + c.var_cam;
    }
    na += __popcll(am);
  }

  const double *dr = c.drone + b * D2D_JERK_DF;
  d2d_jerk_env e = {{dr[0], dr[1]}, {dr[3], dr[4]}, {dr[5], dr[6]}, {c.target[2 * b], c.target[2 * b + 1]},
                    c.dmap + b * d2d_jerk_grid_bytes(c.W, c.H, c.grid_tile), trk, cap, na, 1.0 / c.scale, c.drone_radius + 10.0};

  // ---- costs, ranks by (cost, index), the tie table ----
  const double pm = d2d_jerk_mod360(d2d_jerk_phi(e.p0[0], e.p0[1], e.g[0], e.g[1]));
  for (int i = lane; i < NT; i += WAVE) {
    cost[i] = d2d_jerk_cost(i, pm);
    order[i] = i;
    seen[i] = 0;
  }
  __syncthreads();
  if (pm == pm) {
    int rank[2] = {0, 0};
    for (int u = 0, i = lane; i < NT; i += WAVE, ++u) {
      const double ci = cost[i];
      int r = 0;
      for (int j = 0; j < NT; ++j) {
        const double cj = cost[j];
        r += (cj < ci || (cj == ci && j < i)) ? 1 : 0;
      }
      rank[u] = r;                                     // a permutation of 0 .. 71: the costs are not NaN
    }
    __syncthreads();
    for (int u = 0, i = lane; i < NT; i += WAVE, ++u) order[rank[u]] = i;
  }
  __syncthreads();
  const int pat = d2d_jerk_pattern(pm);
  const uint8_t *perm = c.tie_perm + (size_t)pat * NT, *eq = c.tie_eq + (size_t)pat * NT;
  bool fits = true, tied = false;
  for (int r = lane; r < NT; r += WAVE) {
    const int t0 = perm[r], t1 = r + 1 < NT ? perm[r + 1] : 0;
    if (t0 >= NT || t1 >= NT) {
      fits = false;
    } else {
      atomicAdd(&seen[t0], 1);
      if (r + 1 < NT) {
        const double x = cost[t0], y = cost[t1];
        if (!(eq[r] ? x == y : x < y)) fits = false;
      }
    }
    if (r + 1 < NT) tied = tied || cost[order[r]] == cost[order[r + 1]];
  }
  __syncthreads();
  for (int r = lane; r < NT; r += WAVE) fits = fits && seen[r] == 1;
  const bool use_table = __ballot(!fits) == 0ull;
  int stat = 0;
  if (!use_table && (__ballot(tied) != 0ull || pm != pm)) stat |= D2D_JERK_STAT_UNKNOWN;
  __syncthreads();
  if (use_table)
    for (int r = lane; r < NT; r += WAVE) order[r] = perm[r];
  __syncthreads();

  // ---- the walk ----
  int found = -1;
  if (S <= WAVE) {
    const int per = WAVE / S, q = lane / S, s = lane - q * S;
    const unsigned long long ones = S == WAVE ? ~0ull : (1ull << S) - 1ull;
    for (int r0 = 0; r0 < NT && found < 0; r0 += per) {
      const int r = r0 + q;
      bool bad = false;
      if (q < per && r < NT) {
        const int th = order[r];
        if (s < d2d_jerk_times(&c, th)) {
          d2d_jerk_prim pr;
          d2d_jerk_primitive(c.th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c.half_v_max, &pr);
          bad = !d2d_jerk_sample_free(&c, &e, &pr, th, s);
        }
      }
      const unsigned long long bm = __ballot(bad);
      for (int u = 0; u < per && r0 + u < NT; ++u)
        if (((bm >> (u * S)) & ones) == 0ull) {
          found = r0 + u;
          break;
        }
    }
  } else {
    for (int r = 0; r < NT && found < 0; ++r)
      if (prim_free(c, e, order[r], lane)) found = r;
  }
  const int th = found >= 0 ? order[found] : -1;
  if (found >= 0 && found + 1 < NT && cost[order[found + 1]] == cost[th] && prim_free(c, e, order[found + 1], lane))
    stat |= D2D_JERK_STAT_TIE;

  if (lane == 0) {
    double *wp = c.wp + b * 6;
    if (found >= 0) {
      const double *tt = c.tt_tab + (size_t)th * S * D2D_JERK_TT_F;
      d2d_jerk_prim pr;
      d2d_jerk_primitive(c.th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c.half_v_max, &pr);
      for (int ii = 0; ii < 2; ++ii) {
        wp[ii] = d2d_jerk_pos(&pr, ii, tt, e.p0[ii], e.v0[ii], e.a0[ii]);
        wp[2 + ii] = d2d_jerk_vel(&pr, ii, tt, e.v0[ii], e.a0[ii]);
        wp[4 + ii] = d2d_jerk_acc(&pr, ii, tt, e.a0[ii]);
      }
    } else {
      for (int i = 0; i < 6; ++i) wp[i] = 0.0;
    }
    c.choice[b] = th;
    c.plan_ok[b] = c.wp_valid[b] = found >= 0 ? 1 : 0;
    c.stat[b] = stat | ((found >= 0 ? found + 1 : NT) << D2D_JERK_STAT_SHIFT);
  }
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

}  // namespace

extern "C" {

int d2d_jerk_version(void) { return D2D_JERK_VERSION; }
const char *d2d_jerk_last_error(void) { return g_err; }

int d2d_jerk_plan(const d2d_jerk_call *c, void *stream) {
  if (!c) return fail(-1, "d2d_jerk_plan: call is NULL");
  if (c->B < 1 || c->N < 0 || c->S < 1) return fail(-1, "d2d_jerk_plan: B >= 1, N >= 0, S >= 1");
  if (c->S > D2D_JERK_MAX_S) return failf(-4, "d2d_jerk_plan: S = %d samples a primitive, at most %d", c->S, D2D_JERK_MAX_S);
  if (c->N > D2D_JERK_MAX_N) return failf(-4, "d2d_jerk_plan: N = %d trackers, at most %d fit the wave's LDS", c->N, D2D_JERK_MAX_N);
  if (c->W < 1 || c->H < 1 || c->W > 32767 || c->H > 32767) return fail(-1, "d2d_jerk_plan: 1 <= W, H <= 32767");
  if (c->grid_tile != 0 && c->grid_tile != 16) return fail(-1, "d2d_jerk_plan: grid_tile must be 0 or 16");
  if (!(c->scale > 0.0) || !(c->W_px > 0.0 && c->W_px <= 1e9) || !(c->H_px > 0.0 && c->H_px <= 1e9))
    return fail(-1, "d2d_jerk_plan: scale > 0, 0 < W_px, H_px <= 1e9");
  if (!c->drone || !c->target || !c->dmap) return fail(-1, "d2d_jerk_plan: a state pointer is NULL");
  if (c->N > 0 && (!c->active || !c->kf || !c->trk_radius || !c->trk_prev)) return fail(-1, "d2d_jerk_plan: a tracker pointer is NULL");
  if (!c->th_tab || !c->tt_tab || !c->tie_perm || !c->tie_eq) return fail(-1, "d2d_jerk_plan: a table pointer is NULL");
  if (!c->plan_ok || !c->wp_valid || !c->wp || !c->choice || !c->stat) return fail(-1, "d2d_jerk_plan: an output pointer is NULL");
  const size_t lds = sizeof(double) * 5 * (size_t)(c->N > 0 ? c->N : 1);
  hipLaunchKernelGGL(jerk_plan_kernel, dim3((unsigned)c->B), dim3(WAVE), lds, (hipStream_t)stream, *c);
  return launched("d2d_jerk_plan");
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
