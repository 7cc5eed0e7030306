/*
 * d2d_metrics.h — C ABI of the difficulty metrics on the device (libd2d_metrics.so): the velocity-obstacle feasibility metric,
 * the traversability metric and the survival-fit metric of the reference's script/difficulty_calculator/.
 *
 * The velocity-obstacle feasibility metric of the reference's script/difficulty_calculator/vo_calculator.py:36-120: for a seeded
 * world (the agents' initial positions, preferred velocities and radii), a grid of drone positions and a table of candidate
 * velocities, the number of candidates that lie in no agent's velocity-obstacle cone.
 *
 *   d2d_vo_geometry   :74-85   dist, theta_BA, the collision test        -> arg = (rA + rB) / dist, theta_ba, collided
 *   d2d_vo_cones_arg  :87-91, :107-108   half = asin(arg), the cone's edges -> cone = (theta_right, theta_left), half
 *   (d2d_vo_cones     :88-91, :107-108   the cone's edges from a `half` the caller supplies: the earlier form of that step)
 *   d2d_vo_count      :101-116 the candidates no cone contains           -> count
 *
 * asin is csrc/metrics/d2d_asin.h, a restatement of the host libm's asin that returns its bits (as csrc/ restates sin, cos, atan2,
 * tan, log and pow(x, 2.0)): the whole metric runs on the device, nothing crosses to the host between the launches.
 * d2d_vo_cones is the earlier form of the middle step, with `half` as an INPUT that the caller takes through the host's libm
 * (metrics.host_asin) between d2d_vo_geometry and it; both forms give the same bits.  d2d_asin_array is the test hook of the asin
 * alone.
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
 *
 * Traversability (traversibility_calculator.py -> envs/metric_env.py:286-293 -> demos/traversibility.py:26-51): from each start cell
 * of the ground-truth grid, the cells walked in each of eight directions while the next cell is inside the grid and UNOCCUPIED.
 *
 *   d2d_trav_steps    traversibility.py:32-48   the walks, counted in steps (integers only)    -> steps
 *   (host)            :46, :51, metric_env.py:291-293   a diagonal step is math.sqrt(2), added one at a time; np.mean of the eight
 *                     distances; the running sum over the starts
 *
 * Sizes: B, W, H, S >= 1 with B <= 2^31 - 1, W * H <= 2^31 - 1 and B * S * 8 <= 2^31 - 1 (-4 otherwise).
 *
 * Survival fit (survivability_calculator.py:13-48, the table script/fit.py fits the difficulty model to): the agents move under the
 * constant-velocity model (envs/drone_v2.py:176-179 + utils.py:472-493, which reads neither a grid nor the drone) and every `dt` a
 * drone standing at each of P positions is tested against every agent; the time of the first hit is the position's survival time.
 *
 *   d2d_fit_first_hit  :32-41   one agent update, then `checks` times (test, update)          -> first (the index of the check)
 *   (host)             :30, :34, :40, :45-48   np.arange(0, T, 0.1)[first], min, - 0.1, the clamp, np.mean
 *
 * Sizes: B, N, P >= 1, checks >= 0 with B <= 2^31 - 1, N <= 256 (four tiles of 64 agents, kept in registers over all steps),
 * P <= 64 * 65535 and B * max(P, 6 * N) <= 2^31 - 1 (-4 otherwise).
 */
#ifndef D2D_METRICS_H
#define D2D_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_METRICS_VERSION 2

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

/* d2d_vo_cones with the half angle taken on the device: half = arg > 1 ? 0 : asin(arg) (csrc/metrics/d2d_asin.h), arg as
 * d2d_vo_geometry wrote it.  half_out: [B][P][N] or NULL; it receives the half angle of EVERY pair, those of collided positions
 * included (what metrics.host_asin produces), cone as d2d_vo_cones.  Every entry of cone, and of half_out when given, is written
 * whatever the buffers held.  Sizes and errors as d2d_vo_cones. */
int d2d_vo_cones_arg(const double *theta_ba, const double *arg, const uint8_t *collided, int32_t B, int32_t N, int32_t P,
                     double *half_out, double *cone, void *stream);

/* test hook: out[i] = d2d_asin(x[i]), libm's asin (NaN for NaN and for |x| > 1, where Python's math.asin raises); n >= 0
 * (0: no launch), n <= (2^31 - 1) * 256 (-4 otherwise); out may alias x. */
int d2d_asin_array(const double *x, int64_t n, double *out, void *stream);

/* agents [B][6][N] (rows VX, VY), cand [C][2] (vx, vy), cone, collided -> count [B][P] (i32): the candidates for which no agent's
 * in_between(theta_right, theta_dif, theta_left) holds, or -1 for a collided position.  Every entry is written by the call
 * whatever the buffer held (the call sets them before its counting kernel adds to them). */
int d2d_vo_count(const double *agents, const double *cand, const double *cone, const uint8_t *collided, int32_t B, int32_t N,
                 int32_t P, int32_t C, int32_t *count, void *stream);

#define D2D_TRAV_MAX_ELEMS 0x7fffffff /* W * H, the cells of one grid; B * S * 8, the entries of `steps`; B, a grid dimension */
#define D2D_FIT_MAX_N 256            /* agents of one world: four register tiles of 64 */
#define D2D_FIT_MAX_P (64 * 65535)   /* positions of one call (64 per wave, a grid dimension) */
#define D2D_FIT_MAX_ELEMS 0x7fffffff /* B * P, the entries of `first`; B * 6 * N, the doubles of `agents`; B, a grid dimension */

/* gt [B][W][H] (u8, row-major: the reference's grid_map[i][j], never a tiled layout), starts [S][2] (i32: i, j) -> steps [B][S][8]
 * (i32): the steps walked from (i, j) towards N, NE, E, SE, S, SW, W, NW = (-1,0), (-1,1), (0,1), (1,1), (1,0), (1,-1), (0,-1),
 * (-1,-1) while the next cell is inside the grid and 2 (UNOCCUPIED); -1 in all eight when the start cell is not 2.  Every entry is
 * written whatever the buffer held.  `starts` lives on the device, so the library cannot look at it before the launch: the CALLER
 * refuses a start outside the grid before uploading it (metrics.trav_steps does).  The kernel reads no cell outside the grid
 * whatever `starts` holds; a start outside it gets -1 like any other start that is not an UNOCCUPIED cell. */
int d2d_trav_steps(const uint8_t *gt, int32_t B, int32_t W, int32_t H, const int32_t *starts, int32_t S, int32_t *steps, void *stream);

/* agents [B][6][N] (not modified), pos [P][2] (x, y) -> first [B][P] (i32), agents_out [B][6][N] or NULL.  The agents are updated
 * once; then, `checks` times, every position is tested against every agent (dist < r_j + drone_radius, dist = sqrt(fma(y, y, x * x))
 * as in d2d_vo_geometry) and the agents are updated again.  first = the index of the first check that hit, or -1.  agents_out = the
 * agents after the checks + 1 updates (rows PX, PY; VX, VY = pref_velocity; R and R2 copied): what the reference's env holds when
 * env_metrics returns.  W_px, H_px, scale, dt: params.map_size, map_scale, dt.  Every entry of both outputs is written whatever the
 * buffers held; agents_out must not overlap agents. */
int d2d_fit_first_hit(const double *agents, const double *pos, double drone_radius, double W_px, double H_px, double scale, double dt,
                      int32_t B, int32_t N, int32_t P, int32_t checks, int32_t *first, double *agents_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_METRICS_H */
