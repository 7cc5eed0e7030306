// d2d_gaze.hip — the gaze decision of the step path on the device (gfx950): kernels + the C entry points of include/d2d_gaze.h.  Its
// own library (libd2d_gaze.so): it shares no kernel with the step, the closed loop, the worlds, the metrics, the RVO profile or the
// Jerk_Primitive planner.
//
//   gaze_lookahead  thread = env.  The flag, the velocity and the yaw; one atan2 for a moving drone.
//   gaze_owl        one wave per env, four envs a workgroup, no LDS.
//                   gate        the env's flag, calls left and held rate are requested together, before any of them is looked at: a
//                               finished env ends there, an env that pops its held decision writes two doubles and ends there.
//                               Neither touches a tracker nor calls atan2.
//                   scores      lane = direction (36): update_U.
//                   lookups     lane = candidate (20), lane 20 = the goal direction, lane 21 = the flight direction: U.
//                   trackers    64 list entries a pass, lane = entry: the entry's direction (one atan2 a lane) and weight; the
//                               candidates then add the entries in list order, the values handed round by shuffles.
//                   costs       lane = candidate; np.argmin by a walk over 20 shuffles; lane 0 writes.
//   gaze_reset      thread = one double of the Owl state.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_gaze.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_GAZE_QUAL __device__ __forceinline__
#define D2D_ATAN2_QUAL __device__ __forceinline__
#define D2D_ATAN2_TBL_QUAL __device__ const
#define D2D_POW2_QUAL __device__ __forceinline__
#define D2D_POW2_TBL_QUAL __device__ const
#include "d2d_gaze.h"

#define WAVE 64
#define EW_BLOCK 256
#define OWL_WAVES 4

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

__device__ __forceinline__ double shfl_f64(double v, int src) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = __shfl((unsigned)b, src, WAVE), hi = __shfl((unsigned)(b >> 32), src, WAVE);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(EW_BLOCK) void gaze_lookahead_kernel(const d2d_gaze_call c) {
  const long long b = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (b >= c.B) return;
  const double *dr = c.drone + (size_t)b * D2D_GAZE_DF;
  const int done = c.flags ? c.flags[(size_t)b * 4 + D2D_GAZE_F_DONE] : 0;
  const double yaw = dr[2], vx = dr[3], vy = dr[4];
  if (done) return;
  c.action[b] = d2d_gaze_lookahead(vx, vy, yaw, c.dt, c.yaw_rate_max);
}

__global__ __launch_bounds__(OWL_WAVES *WAVE) void gaze_owl_kernel(const d2d_gaze_call c) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long e = (long long)blockIdx.x * OWL_WAVES + (threadIdx.x >> 6);
  if (e >= c.B) return;
  double *st = c.owl_state + (size_t)e * D2D_GAZE_OWL_STATE_F;
  const double *__restrict__ tab = c.owl_tab;

  // ---- gate: one batch of loads ----
  const int done = c.flags ? c.flags[(size_t)e * 4 + D2D_GAZE_F_DONE] : 0;
  const double left = st[D2D_GAZE_OWL_S_LEFT], held = st[D2D_GAZE_OWL_S_RATE];
  if (done) return;
  if (left > 0.0) {  // `if len(self.u) != 0: return self.u.pop() / top`
    if (lane == 0) {
      st[D2D_GAZE_OWL_S_LEFT] = left - 1.0;
      c.action[e] = held / c.yaw_rate_max;
    }
    return;
  }

  // ---- a decision: everything that does not hang on another load is requested here ----
  const double *dr = c.drone + (size_t)e * D2D_GAZE_DF;
  const double x0 = dr[0], y0 = dr[1], yaw = dr[2], vx = dr[3], vy = dr[4];
  const double tx = c.target[(size_t)e * 2], ty = c.target[(size_t)e * 2 + 1];
  const double half = tab[D2D_GAZE_T_FOV] * 0.5, depth = tab[D2D_GAZE_T_DEPTH];
  const int cand = lane < D2D_GAZE_NRATE ? lane : D2D_GAZE_NRATE - 1;
  const double r08 = tab[D2D_GAZE_T_RATE08 + cand], turn = tab[D2D_GAZE_T_TURN + cand];
  const double old = lane < D2D_GAZE_NDIR ? st[lane] : 0.0;
  const int N = c.N;
  const uint8_t *act = c.active + (size_t)e * N;
  const double *kf = c.kf + (size_t)e * N * D2D_GAZE_KF;
  const double hp = d2d_gaze_mod360(half), hn = d2d_gaze_mod360(-half);

  // update_U (:175-181): lane k < 36 owns direction 10 k degrees
  double sc_l = 0.0;
  if (lane < D2D_GAZE_NDIR) {
    sc_l = d2d_gaze_score(old, lane, vx, vy, d2d_gaze_mod360(-yaw), tab, half, depth);
    st[lane] = sc_l;
  }

  // d_g (lane 20) and d_v (every other lane; lane 21's is used), :200-201
  const double vn = d2d_gaze_norm(vx, vy);
  const double ang = d2d_atan2(lane == 20 ? ty - y0 : vy / vn, lane == 20 ? tx - x0 : vx / vn) * D2D_GAZE_RAD2DEG;
  const double d_g = shfl_f64(ang, 20), d_v = shfl_f64(ang, 21);

  // U(theta) (:183-185) for the candidates' headings (lanes 0..19), d_g (lane 20) and d_v (lane 21)
  const double h = -(yaw + r08);
  const int near = d2d_gaze_nearest(d2d_gaze_mod360(lane < D2D_GAZE_NRATE ? h : (lane == 20 ? d_g : d_v)));
  const double u_l = shfl_f64(sc_l, near);
  const double goal_unknown = 1.0 - shfl_f64(u_l, 20), flight_unknown = 1.0 - shfl_f64(u_l, 21);

  // f[i, 0], f[i, 1] (:208-209)
  const double t0 = d2d_gaze_unseen(h - d_g, half, hp, hn) * goal_unknown;
  const double speed2 = d2d_pow2(d2d_gaze_norm(vx / 10.0, vy / 10.0));
  const double t1 = (speed2 * d2d_gaze_unseen(h - d_v, half, hp, hn)) * flight_unknown;

  // f[i, 2] (:211-212): d_o lists the ACTIVE trackers in index order; zip(d_o, trackers) weights the j-th of them with the state of
  // tracker j.  Every pass walks the active bytes once, 64 at a time, and lane l keeps the index of list entry j0 + l.
  int nact = 0;
  for (int b0 = 0; b0 < N; b0 += WAVE) {
    const int t = b0 + lane;
    nact += __popcll(__ballot(t < N && act[t] != 0));
  }
  double t2 = 0.0;
  for (int j0 = 0; j0 < nact; j0 += WAVE) {
    const int j = j0 + lane;
    int mine = 0, seen = 0;
    for (int b0 = 0; b0 < N && seen < j0 + WAVE; b0 += WAVE) {
      const int t = b0 + lane;
      const unsigned long long m = __ballot(t < N && act[t] != 0);
      const int cnt = __popcll(m);
      if (j >= seen && j < seen + cnt) {  // the (j - seen)-th set bit of m
        unsigned long long r = m;
        for (int q = j - seen; q > 0; --q) r &= r - 1;
        mine = b0 + __ffsll((long long)r) - 1;
      }
      seen += cnt;
    }
    double d_o = 0.0, pull = 0.0;
    if (j < nact) {  // mine < N and j < nact <= N
      d_o = d2d_gaze_agent_dir(kf + (size_t)mine * D2D_GAZE_KF, x0, y0);
      pull = d2d_gaze_agent_pull(kf + (size_t)j * D2D_GAZE_KF, x0, y0);
    }
    const int cnt = min(nact - j0, WAVE);
    for (int q = 0; q < cnt; ++q) t2 += shfl_f64(pull, q) * d2d_gaze_unseen(h - shfl_f64(d_o, q), half, hp, hn);
  }

  const double cost = d2d_gaze_cost(t0, t1, t2, u_l, turn);

  // np.argmin (:218)
  int best = 0;
  double best_c = shfl_f64(cost, 0);
  for (int a = 1; a < D2D_GAZE_NRATE; ++a) {
    const double v = shfl_f64(cost, a);
    if (d2d_gaze_better(v, best_c)) {
      best = a;
      best_c = v;
    }
  }
  if (lane == 0) {
    st[D2D_GAZE_OWL_S_RATE] = tab[D2D_GAZE_T_RATE + best];
    st[D2D_GAZE_OWL_S_LEFT] = tab[D2D_GAZE_T_HOLD];
    c.action[e] = tab[D2D_GAZE_T_ACT + best];
  }
}

__global__ __launch_bounds__(EW_BLOCK) void gaze_reset_kernel(double *__restrict__ owl_state, const uint8_t *__restrict__ mask,
                                                             int mask_stride, long long total) {
  const long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x;
  if (t >= total) return;
  if (mask && !mask[(size_t)(t / D2D_GAZE_OWL_STATE_F) * mask_stride]) return;
  owl_state[t] = 0.0;
}

int launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  return failf(-3, "%s: launch failed: %s", who, hipGetErrorString(err));
}

}  // namespace

extern "C" {

int d2d_gaze_version(void) { return D2D_GAZE_VERSION; }
const char *d2d_gaze_last_error(void) { return g_err; }

int d2d_gaze_act(const d2d_gaze_call *c, void *stream) {
  if (!c) return fail(-1, "d2d_gaze_act: call is NULL");
  if (c->B < 1 || c->N < 0) return fail(-1, "d2d_gaze_act: B >= 1, N >= 0");
  if (c->N > D2D_GAZE_MAX_N) return failf(-4, "d2d_gaze_act: N = %d trackers, at most %d", c->N, D2D_GAZE_MAX_N);
  if (c->kind != D2D_GAZE_K_LOOKAHEAD && c->kind != D2D_GAZE_K_OWL)
    return failf(-1, "d2d_gaze_act: kind %d: D2D_GAZE_K_LOOKAHEAD (%d) or D2D_GAZE_K_OWL (%d)", c->kind, D2D_GAZE_K_LOOKAHEAD, D2D_GAZE_K_OWL);
  if (!(c->dt > 0.0) || !(c->yaw_rate_max > 0.0)) return fail(-1, "d2d_gaze_act: dt > 0, yaw_rate_max > 0");
  if (!c->drone || !c->action) return fail(-1, "d2d_gaze_act: drone or action is NULL");
  if (c->kind == D2D_GAZE_K_LOOKAHEAD) {
    hipLaunchKernelGGL(gaze_lookahead_kernel, dim3((unsigned)((c->B + EW_BLOCK - 1) / EW_BLOCK)), dim3(EW_BLOCK), 0, (hipStream_t)stream, *c);
    return launched("d2d_gaze_act");
  }
  if (!c->target || !c->owl_state || !c->owl_tab) return fail(-1, "d2d_gaze_act: Owl needs target, owl_state and owl_tab");
  if (c->N > 0 && (!c->active || !c->kf)) return fail(-1, "d2d_gaze_act: a tracker pointer is NULL");
  hipLaunchKernelGGL(gaze_owl_kernel, dim3((unsigned)((c->B + OWL_WAVES - 1) / OWL_WAVES)), dim3(OWL_WAVES * WAVE), 0, (hipStream_t)stream, *c);
  return launched("d2d_gaze_act");
}

int d2d_gaze_reset(double *owl_state, const uint8_t *mask, int32_t mask_stride, int32_t B, void *stream) {
  if (B < 1 || mask_stride < 1) return fail(-1, "d2d_gaze_reset: B >= 1, mask_stride >= 1");
  if (!owl_state) return fail(-1, "d2d_gaze_reset: owl_state is NULL");
  const long long total = (long long)B * D2D_GAZE_OWL_STATE_F;
  hipLaunchKernelGGL(gaze_reset_kernel, dim3((unsigned)((total + EW_BLOCK - 1) / EW_BLOCK)), dim3(EW_BLOCK), 0, (hipStream_t)stream,
                     owl_state, mask, (int)mask_stride, total);
  return launched("d2d_gaze_reset");
}

}  // extern "C"
