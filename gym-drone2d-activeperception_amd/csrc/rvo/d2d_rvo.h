/*
 * d2d_rvo.h — per-element arithmetic of the RVO motion profile (include/d2d_rvo.h names the reference lines).
 *
 * The reference (utils.py:299-460) decides, for agent A at pA with current velocity vA and preferred velocity pref:
 *
 *   ROB_RAD   = agents[0].radius + 0.01                       one value for every agent of the env
 *   per other agent B (pB, vB):
 *     apex      = pA + 0.5 * (vB + vA)
 *     dist      = numpy.linalg.norm(pA - pB)                   sqrt(fma(y, y, x * x)), d2d_vo_norm; raised to rad where below it
 *     rad       = 2 * ROB_RAD
 *     theta_BA  = math.atan2(pB.y - pA.y, pB.x - pA.x)
 *     half      = math.asin(rad / dist)                        <= asin(1): the clamp keeps the argument in (0, 1]
 *     left      = math.atan2(sin(theta_BA + half), cos(theta_BA + half))    intersect() re-evaluates these two per candidate;
 *     right     = math.atan2(sin(theta_BA - half), cos(theta_BA - half))    they are constants of the cone
 *   per pillar (x, y, r): apex = pA + 0, rad = r * 1.5 + ROB_RAD, the rest alike
 *   candidates: rad * (cos theta, sin theta), theta over np.arange(0, 2 * 3.14, 0.2) (32 values: D2D_RVO_COS / _SIN hold libm's
 *     cos / sin of i * 0.2), rad over np.arange(0.02, |pref| + 0.02, |pref| / 5.0) (d2d_rvo_radii: numpy's length and fill rule);
 *     theta-major, and pref itself last
 *   a candidate v lies in a cone iff in_between(right, atan2(v.y + pA.y - apex.y, v.x + pA.x - apex.x), left)  (d2d_vo_in_between)
 *   some candidate in no cone: the first such candidate with the smallest norm(v - pref)
 *   none: per candidate tc = min over its cones of d2d_rvo_tc (Python's min: a NaN stays only at the front of the list); the first
 *     candidate with the smallest 0.2 / (tc + 0.001) + norm(v - pref), where a NaN key wins only as candidate 0
 *
 * The candidates are distinct 2-vectors, so the reference's dict keyed by the candidate's value (utils.py:405-431) holds one entry
 * per candidate.
 *
 * Must be compiled with -ffp-contract=off: every '*' '+' '-' '/' is one IEEE-754 binary64 operation, every D2D_FMA one fused
 * multiply-add.  The scalar pieces are shared by the device kernels (d2d_rvo.hip) and by the plain loops at the end of this file
 * (host builds only), which the CPU tests compare with a Python model bit for bit.
 */
#ifndef D2D_RVO_IMPL_H
#define D2D_RVO_IMPL_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/d2d.h" /* D2D_AF, D2D_A_*: the rows of the state's agents [6][N] */
#include "../../../include/d2d_rvo.h"

#ifndef D2D_RVO_QUAL
#define D2D_RVO_QUAL static inline
#endif
#ifndef D2D_RVO_TBL_QUAL
#define D2D_RVO_TBL_QUAL static const
#endif
#ifndef D2D_VO_QUAL
#define D2D_VO_QUAL D2D_RVO_QUAL
#endif
#include "../metrics/d2d_vo.h" /* d2d_vo_norm, d2d_vo_in_between; d2d_atan2.h, d2d_sincos.h, d2d_asin.h */

#define D2D_RVO_NTHETA 32 /* len(np.arange(0, 2 * 3.14, 0.2)) = ceil(6.28 / 0.2); element i is 0 + i * 0.2 */
#define D2D_RVO_CONE_F 6  /* doubles of one cone */
#define D2D_RVO_C_AX 0
#define D2D_RVO_C_AY 1
#define D2D_RVO_C_RIGHT 2
#define D2D_RVO_C_LEFT 3
#define D2D_RVO_C_DIST 4
#define D2D_RVO_C_RAD 5

/* math.cos / math.sin of i * 0.2, i = 0 .. 31, as the host's libm returns them */
D2D_RVO_TBL_QUAL double D2D_RVO_COS[D2D_RVO_NTHETA] = {
    0x1.0000000000000p+0,  0x1.f5cb49577627ap-1,  0x1.d7954e7dba2f8p-1,  0x1.a69263c485b14p-1,
    0x1.64b6bde719865p-1,  0x1.14a280fb5068cp-1,  0x1.730de943b79d0p-2,  0x1.5c17bbc135703p-3,
    -0x1.de67ac55f1633p-6, -0x1.d14f54f250e7ap-3, -0x1.aa22657537205p-2, -0x1.2d5004b88ad70p-1,
    -0x1.798bab490d188p-1, -0x1.b6ba1f680f470p-1, -0x1.e26af7757704cp-1, -0x1.fae04be85e5d2p-1,
    -0x1.ff207e2b9cbb6p-1, -0x1.ef002c35ebe02p-1, -0x1.cb23eb4d22c59p-1, -0x1.94f9b84dba8e8p-1,
    -0x1.4eaa606db24c1p-1, -0x1.f606eec8ac71dp-2, -0x1.3ab577c62c2aap-2, -0x1.cb6072b598d8ap-4,
    0x1.66655584e407fp-4,  0x1.22785706b4ad9p-2,  0x1.dfc2d59376aeep-2,  0x1.44f676f25b08cp-1,
    0x1.8d16f88830a84p-1,  0x1.c562d06a77227p-1,  0x1.eb9b7097822f5p-1,  0x1.fe3ac4079a9cep-1};
D2D_RVO_TBL_QUAL double D2D_RVO_SIN[D2D_RVO_NTHETA] = {
    0x0.0p+0,              0x1.96dff233dd2bcp-3,  0x1.8ec3ae92b676bp-2,  0x1.2118d17a5415ap-1,
    0x1.6f494c2bffecdp-1,  0x1.aed548f090ceep-1,  0x1.dd343a21a55c5p-1,  0x1.f88cddf44e103p-1,
    0x1.ffc81c7e042c5p-1,  0x1.f29c281bd15f0p-1,  0x1.d18f6ead1b446p-1,  0x1.9df33d9aad708p-1,
    0x1.59d64f5c3d198p-1,  0x1.07efcbba085bbp-1,  0x1.57072235de5c0p-2,  0x1.210386db6d55bp-3,
    -0x1.de33739e82d32p-5, -0x1.05ac910ff4c74p-2, -0x1.c524143f0d1f1p-2, -0x1.39456ffecc0a0p-1,
    -0x1.837b9dddc1eaep-1, -0x1.be3f2dfd012d8p-1, -0x1.e7386314528efp-1, -0x1.fcc51135decbap-1,
    -0x1.fe0949a0c3dffp-1, -0x1.eaf81f5e09933p-1, -0x1.c4542b2ba24d7p-1, -0x1.8ba7c97320570p-1,
    -0x1.433561796f5b4p-1, -0x1.dbc0ac78edfcap-2, -0x1.1e1f18ab0a2c0p-2, -0x1.54558dbbecd1dp-4};

/* utils.py:320-332 (an agent: apex = pA + 0.5 * (vB + vA), rad = 2 * ROB_RAD) and :338-351 (a pillar: apex = pA + 0,
 * rad = r * 1.5 + ROB_RAD): the caller passes apex and rad.  c: the cone's six doubles, `stride` apart. */
D2D_RVO_QUAL void d2d_rvo_cone(double pax, double pay, double pbx, double pby, double apx, double apy, double rad, double *c,
                               size_t stride) {
  double dist = d2d_vo_norm(pax - pbx, pay - pby);
  const double theta = d2d_atan2(pby - pay, pbx - pax);
  if (rad > dist) dist = rad;
  const double half = d2d_asin(rad / dist);
  const double l = theta + half, r = theta - half;
  c[D2D_RVO_C_AX * stride] = apx;
  c[D2D_RVO_C_AY * stride] = apy;
  c[D2D_RVO_C_RIGHT * stride] = d2d_atan2(d2d_sin(r), d2d_cos(r));
  c[D2D_RVO_C_LEFT * stride] = d2d_atan2(d2d_sin(l), d2d_cos(l));
  c[D2D_RVO_C_DIST * stride] = dist;
  c[D2D_RVO_C_RAD * stride] = rad;
}

/* cone k of agent i among the N - 1 + P cones of its env: the other agents in index order, then the pillars.  ag: the env's agents
 * [6][N], vel [2][N], pil [P][3] */
D2D_RVO_QUAL void d2d_rvo_cone_of(const double *ag, const double *vel, const int32_t *pil, int N, int i, int k, double rob_rad,
                                  double *c, size_t stride) {
  const double pax = ag[D2D_A_PX * N + i], pay = ag[D2D_A_PY * N + i];
  if (k < N - 1) {
    const int j = k < i ? k : k + 1;
    const double vax = vel[i], vay = vel[N + i], vbx = vel[j], vby = vel[N + j];
    d2d_rvo_cone(pax, pay, ag[D2D_A_PX * N + j], ag[D2D_A_PY * N + j], pax + 0.5 * (vbx + vax), pay + 0.5 * (vby + vay), 2 * rob_rad,
                 c, stride);
  } else {
    const int32_t *h = pil + 3 * (size_t)(k - (N - 1));
    d2d_rvo_cone(pax, pay, (double)h[0], (double)h[1], pax + 0.0, pay + 0.0, (double)h[2] * 1.5 + rob_rad, c, stride);
  }
}

/* np.arange(0.02, norm_v + 0.02, norm_v / 5.0): the length ceil((stop - start) / step) -- 5 for almost every speed, 6 for a few --
 * and *delta = (start + step) - start; element r is 0.02 + r * delta.  A speed of 0 (which the reference cannot run: np.arange
 * raises, and the host refuses it) gives no radius here: the only candidate is pref. */
D2D_RVO_QUAL int d2d_rvo_radii(double norm_v, double *delta) {
  const double start = 0.02, stop = norm_v + 0.02, step = norm_v / 5.0;
  const double val = (stop - start) / step;
  *delta = (start + step) - start;
  if (!(val > 0.0)) return 0;
  return (int)__builtin_ceil(val < 64.0 ? val : 64.0); /* (val stays below 12 for every speed a double can hold) */
}

/* candidate c of 32 * nrad + 1: theta-major, then rad, pref last */
D2D_RVO_QUAL void d2d_rvo_candidate(int c, int nrad, double delta, double prefx, double prefy, double *cx, double *cy) {
  if (c >= D2D_RVO_NTHETA * nrad) {
    *cx = prefx;
    *cy = prefy;
    return;
  }
  const int t = c / nrad, r = c - t * nrad;
  const double rad = 0.02 + (double)r * delta;
  *cx = rad * D2D_RVO_COS[t];
  *cy = rad * D2D_RVO_SIN[t];
}

/* utils.py:371-374 / :415-419: does candidate (cx, cy) of the agent at pA lie in the cone?  td, dx, dy: theta_dif and dif */
D2D_RVO_QUAL int d2d_rvo_inside(double cx, double cy, double pax, double pay, double apx, double apy, double right, double left,
                                double *td, double *dx, double *dy) {
  *dx = cx + pax - apx;
  *dy = cy + pay - apy;
  *td = d2d_atan2(*dy, *dx);
  return d2d_vo_in_between(right, *td, left);
}

/* utils.py:420-427: the time-to-collision term of a candidate inside a cone; 0 / 0 = NaN when dif is exactly zero */
D2D_RVO_QUAL double d2d_rvo_tc(double td, double dx, double dy, double right, double left, double dist, double rad) {
  const double small_theta = __builtin_fabs(td - 0.5 * (left + right));
  const double s = __builtin_fabs(dist * d2d_sin(small_theta));
  if (s >= rad) rad = s;
  const double big_theta = d2d_asin(s / rad);
  double dist_tg = __builtin_fabs(dist * d2d_cos(small_theta)) - __builtin_fabs(rad * d2d_cos(big_theta));
  if (dist_tg < 0.0) dist_tg = 0.0;
  return dist_tg / d2d_vo_norm(dx, dy);
}

/* utils.py:431: the key of a candidate that lies in a cone, tc = Python's min over its cones */
D2D_RVO_QUAL double d2d_rvo_key(double tc, double cx, double cy, double prefx, double prefy) {
  return 0.2 / (tc + 0.001) + d2d_vo_norm(cx - prefx, cy - prefy);
}

/* Agent.step (utils.py:472-493) with `velocity` (vx, vy) and `pref_velocity` as separate arrays, which is what RVO_update leaves:
 * the branch of oracle/d2d_oracle.c's st_agents where the two do not alias.  The stuck test reads the velocity, the rotation and
 * the boundary flips change pref, the position moves with the velocity. */
D2D_RVO_QUAL void d2d_rvo_agent_step(double *px, double *py, double *prefx, double *prefy, double vx, double vy, double r, double W_px,
                                     double H_px, double scale, double dt) {
  const double cs = 0x1.bb67ae8584cabp-1, sn = 0x1.fffffffffffffp-2; /* cos(pi/6), sin(pi/6) as numpy returns them */
  const double nx = *px + vx * dt, ny = *py + vy * dt;
  double fx = *prefx, fy = *prefy;
  if (d2d_vo_norm(vx, vy) <= 5.0) {
    /* numpy 2x2 @ 2x1: fma(M[r][0], v0, M[r][1] * v1) */
    const double rx = D2D_FMA(cs, fx, (-sn) * fy), ry = D2D_FMA(sn, fx, cs * fy);
    fx = rx;
    fy = ry;
  }
  if (nx < scale + r) fx = __builtin_fabs(fx);
  else if (nx > W_px - scale - r) fx = -__builtin_fabs(fx);
  if (ny < scale + r) fy = __builtin_fabs(fy);
  else if (ny > H_px - scale - r) fy = -__builtin_fabs(fy);
  *px = nx;
  *py = ny;
  *prefx = fx;
  *prefy = fy;
}

#if !defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
/* ---- the entry points as plain loops over host arrays (tests/csrc/rvo_host.c), same layouts as include/d2d_rvo.h ---- */

/* `work`: 6 * (N - 1 + P) doubles of scratch (the cones of one agent); returns 0, or -4 above D2D_RVO_MAX_CONES */
D2D_RVO_QUAL int d2d_rvo_velocity_seq(const double *agents, const double *vel, const int32_t *pillars, int B, int N, int P,
                                      double *vel_out, double *work) {
  const int nc = N - 1 + P;
  if (N > 0 && nc > D2D_RVO_MAX_CONES) return -4;
  for (int b = 0; b < B; ++b) {
    const double *ag = agents + (size_t)b * D2D_AF * N, *v = vel + (size_t)b * 2 * N;
    const int32_t *pil = pillars + (size_t)b * P * 3;
    double *out = vel_out + (size_t)b * 2 * N;
    for (int i = 0; i < N; ++i) {
      const double rob_rad = ag[D2D_A_R * N] + 0.01;
      const double pax = ag[D2D_A_PX * N + i], pay = ag[D2D_A_PY * N + i];
      const double prefx = ag[D2D_A_VX * N + i], prefy = ag[D2D_A_VY * N + i];
      for (int k = 0; k < nc; ++k) d2d_rvo_cone_of(ag, v, pil, N, i, k, rob_rad, work + k, (size_t)nc);
      double delta;
      const int nrad = d2d_rvo_radii(d2d_vo_norm(prefx, prefy), &delta);
      const int C = D2D_RVO_NTHETA * nrad + 1;
      int best = -1;
      double best_key = 0.0;
      for (int c = 0; c < C; ++c) { /* min(suitable_V, key=norm(v - pref)) */
        double cx, cy, td, dx, dy;
        int suit = 1;
        d2d_rvo_candidate(c, nrad, delta, prefx, prefy, &cx, &cy);
        for (int k = 0; k < nc && suit; ++k)
          if (d2d_rvo_inside(cx, cy, pax, pay, work[k], work[nc + k], work[2 * nc + k], work[3 * nc + k], &td, &dx, &dy)) suit = 0;
        if (!suit) continue;
        const double key = d2d_vo_norm(cx - prefx, cy - prefy);
        if (best < 0 || key < best_key) best = c, best_key = key;
      }
      if (best < 0)
        for (int c = 0; c < C; ++c) { /* min(unsuitable_V, key=0.2 / tc_V + norm(v - pref)) */
          double cx, cy, td, dx, dy, tc = 0.0;
          int have = 0;
          d2d_rvo_candidate(c, nrad, delta, prefx, prefy, &cx, &cy);
          for (int k = 0; k < nc; ++k)
            if (d2d_rvo_inside(cx, cy, pax, pay, work[k], work[nc + k], work[2 * nc + k], work[3 * nc + k], &td, &dx, &dy)) {
              const double t = d2d_rvo_tc(td, dx, dy, work[2 * nc + k], work[3 * nc + k], work[4 * nc + k], work[5 * nc + k]);
              if (!have || t < tc) tc = t;
              have = 1;
            }
          const double key = d2d_rvo_key(tc, cx, cy, prefx, prefy);
          if (best < 0 || key < best_key) best = c, best_key = key;
        }
      d2d_rvo_candidate(best, nrad, delta, prefx, prefy, out + i, out + N + i);
    }
  }
  return 0;
}

D2D_RVO_QUAL void d2d_rvo_agents_step_seq(double *agents, const double *vel, double W_px, double H_px, double scale, double dt, int B,
                                          int N) {
  for (int b = 0; b < B; ++b) {
    double *ag = agents + (size_t)b * D2D_AF * N;
    const double *v = vel + (size_t)b * 2 * N;
    for (int i = 0; i < N; ++i)
      d2d_rvo_agent_step(ag + D2D_A_PX * N + i, ag + D2D_A_PY * N + i, ag + D2D_A_VX * N + i, ag + D2D_A_VY * N + i, v[i], v[N + i],
                         ag[D2D_A_R * N + i], W_px, H_px, scale, dt);
  }
}
#endif

#endif /* D2D_RVO_IMPL_H */
