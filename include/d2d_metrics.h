/*
 * d2d_metrics.h — C ABI of the difficulty metrics on the device (libd2d_metrics.so).
 *
 * The velocity-obstacle feasibility metric of the reference's script/difficulty_calculator/vo_calculator.py:36-120: for a seeded
 * world (the agents' initial positions, preferred velocities and radii), a grid of drone positions and a table of candidate
 * velocities, the number of candidates that lie in no agent's velocity-obstacle cone.
 *
 *   d2d_vo_geometry   :74-85   dist, theta_BA, the collision test        -> arg = (rA + rB) / dist, theta_ba, collided
 *   (host)            :87      half = asin(arg) through the host's libm, over the flat array
 *   d2d_vo_cones      :88-91, :107-108   the cone's edges                -> cone = (theta_right, theta_left)
 *   d2d_vo_count      :101-116 the candidates no cone contains           -> count
 *
 * `half` is an INPUT of d2d_vo_cones because the device has no bit-exact restatement of libm's asin yet (csrc/ restates sin,
 * cos, atan2, tan, log and pow(x, 2.0)); everything else of the metric runs on the device.  A later change that adds one can drop
 * the round trip without touching d2d_vo_geometry, d2d_vo_cones' arithmetic or d2d_vo_count.
 *
 * theta_dif = atan2(v.y - vB.y, v.x - vB.x) of vo_calculator.py:106 depends on the candidate and the agent only: d2d_vo_count
 * evaluates it once per (world, candidate, agent) and chunk of positions, not per position.  The script's `break` at :111 only
 * saves time (the result is an OR over the agents), so the evaluation order is free.
 *
 * Conventions as in d2d_worlds.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 bad argument, -3 HIP launch error, -4 unsupported size) with a thread-local message.  The library is
 * separate from libd2d_hip.so and libd2d_worlds.so and reports its own version; no struct of d2d.h is involved: `agents` is the
 * state's own d2d_state.agents, [B][6][N] doubles (rows D2D_A_PX, PY, VX, VY, R, R2).
 *
 * Sizes: any B, N, P, C >= 1 with B <= 65535, P <= 64 * 65535 and B * P * N * 2 < 2^31 (-4 otherwise).
 */
#ifndef D2D_METRICS_H
#define D2D_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_METRICS_VERSION 1

#define D2D_VO_MAX_B 65535           /* worlds of one call (a grid dimension) */
#define D2D_VO_MAX_P (64 * 65535)    /* positions of one call (64 per workgroup, a grid dimension) */
#define D2D_VO_MAX_ELEMS 0x7fffffff  /* B * P * N * 2, the doubles of `cone` */

int d2d_metrics_version(void);
const char *d2d_metrics_last_error(void);

/* agents [B][6][N], pos [P][2] (x, y) -> arg [B][P][N] = (rA + r_j) / dist, theta_ba [B][P][N], collided [B][P] (u8: 1 iff any
 * agent has dist < rA + r_j).  dist = sqrt(fma(y, y, x * x)), x = pA.x - pB.x, y = pA.y - pB.y: numpy's norm of a 2-vector.
 * Every pair is evaluated, also those of collided positions (the reference stops at the first hit and never reads the rest). */
int d2d_vo_geometry(const double *agents, const double *pos, double rA, int32_t B, int32_t N, int32_t P, double *arg,
                    double *theta_ba, uint8_t *collided, void *stream);

/* theta_ba, half [B][P][N], collided [B][P] -> cone [B][P][N][2] = (theta_right, theta_left) = atan2(sin, cos)(theta_ba -+ half);
 * (0, 0) for every agent of a collided position. */
int d2d_vo_cones(const double *theta_ba, const double *half, const uint8_t *collided, int32_t B, int32_t N, int32_t P, double *cone,
                 void *stream);

/* agents [B][6][N] (rows VX, VY), cand [C][2] (vx, vy), cone, collided -> count [B][P] (i32): the candidates for which no agent's
 * in_between(theta_right, theta_dif, theta_left) holds, or -1 for a collided position.  Every entry is written by the call
 * whatever the buffer held (the call sets them before its counting kernel adds to them). */
int d2d_vo_count(const double *agents, const double *cand, const double *cone, const uint8_t *collided, int32_t B, int32_t N,
                 int32_t P, int32_t C, int32_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_METRICS_H */
