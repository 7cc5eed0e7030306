/*
 * d2d_jerk.h — C ABI of the Jerk_Primitive planner on the device (libd2d_jerk.so): the reference's `--planner Jerk_Primitive`
 * (traj_planner.py:403-516), which every step ranks 72 headings by their angular distance to the goal, tests the jerk-optimal
 * primitive of each heading in rank order against the explored map and the active trackers (Planner.is_free, :28-59), and hands the
 * first sample of the first free primitive to step_pos.  It keeps no trajectory between steps: plan() appends one waypoint,
 * step_pos pops it, replan_check always sees an empty list.
 *
 *   d2d_jerk_plan    one call per step, BETWEEN d2d_perceive and d2d_act of include/d2d.h: writes the state's plan_ok, wp_valid, wp
 *                    (the EXTERNAL planner mode's inputs of d2d_act) and the library's own choice / stat
 *   d2d_jerk_reset   the library's per-env tracker bookkeeping back to its start (every env, or those of a mask)
 *
 * What the decision reproduces, operation for operation in fp64 (csrc/jerk/d2d_jerk.h holds the arithmetic):
 *   :472-473   phi_h = math.degrees(math.atan2(dy, dx)) of target - (drone.x, drone.y)
 *   :476-479   cost(theta) = d ** 2 with d = abs(theta % 360 - phi_h % 360), folded to 360 - d above 180; theta = 0, 5 .. 355
 *   :482       the rank order: cost[:, 0].argsort() -- see "ties" below
 *   :414-461   the primitive of a heading: pf = p0 + 30 (cos, sin), vf = (0.5 v_max / norm(l)) l with l = target - pf, af = 0, the
 *              three polynomials at every sample time.  A goal exactly on pf gives norm(l) = 0 and NaN samples, which is_free rejects
 *   :28-59     is_free per sample: NaN test, five get_grid probes at drone_radius + 10 (outside the map counts as occupied), and for
 *              every active tracker norm(p - (mu[:2] + t mu[2:])) <= drone_radius + radius + 5 + var_cam
 *   :495-501   no free primitive: plan_ok = 0, no waypoint.  Else the first sample (position, velocity, acceleration) of the first
 *              free primitive: plan_ok = wp_valid = 1
 *
 * Everything that depends only on (theta, v_max, dt) is a table the HOST builds with numpy's own expressions (cos, sin, ** are the
 * host libm's): no pow, cos or sin runs on the device.
 *   th_tab [72][8]      per heading: delt_x, delt_y, T (after the >= 0.5 clamp), T**2, T**3, T**4, T**5, times (as a double)
 *   tt_tab [72][S][5]   per (heading, sample): tt, tt**2 .. tt**5; rows at and above the heading's `times` are not read
 * `times` differs between headings (17 or 18 at v_max = 20), so S = max(times) is a dimension; 1 <= S <= D2D_JERK_MAX_S.
 *
 * Ties.  A goal on a heading, or exactly midway between two, gives pairs of equal costs, and numpy's default argsort is not stable:
 * which of two tied headings comes first depends on the numpy build and the CPU it dispatches for.  The device ranks by
 * (cost, heading index).  The host then supplies, per weak-order pattern -- goal bin k of 72 x {phi on theta_k, lower half of the
 * bin, exactly midway, upper half} = D2D_JERK_PATTERNS -- the order ITS np.argsort returns for a representative phi:
 *   tie_perm [288][72] u8   heading indices in numpy's order
 *   tie_eq   [288][72] u8   1 where the costs at ranks r and r + 1 of that order are equal in the representative
 * The device uses tie_perm[pattern] where it is a permutation along which the costs at hand rise strictly where tie_eq is 0 and are
 * equal where it is 1: the weak order is then the representative's, and a comparison sort's answer depends on nothing else.
 * Otherwise (rounding ties some pairs and not others, within ~1e-13 degrees of a multiple of 2.5) it keeps (cost, index) order and,
 * if that order holds a tie at all, sets stat bit 1.
 *
 * Tracker bookkeeping as the Primitive planner's (utils.py:184, 238): a tracker that was active and is not any more gets
 * agent_radius back; trk_radius / trk_prev are the library's per-env state, owned by the caller like everything else.
 *
 * Shape: one wave per env.  Costs and ranks with lane = heading; then passes in rank order with the lanes spread over
 * (rank, sample) pairs -- 64 / S primitives a pass -- each of which ballots the free bits; the first pass that holds a fully free
 * primitive ends the walk.  The active trackers of the env are staged in LDS: N <= D2D_JERK_MAX_N.
 *
 * Conventions as in d2d_rvo.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 bad argument, -3 HIP launch error, -4 unsupported size) with a thread-local message.  The library is separate
 * from libd2d_hip.so and reports its own version.
 */
#ifndef D2D_JERK_H
#define D2D_JERK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_JERK_VERSION 1

#define D2D_JERK_NTHETA 72     /* len(np.arange(0, 360, 5)) */
#define D2D_JERK_PATTERNS 288  /* 72 goal bins x 4 kinds */
#define D2D_JERK_MAX_S 128     /* samples of one primitive */
#define D2D_JERK_MAX_N 1024    /* trackers of one env: five doubles each in the wave's LDS */
#define D2D_JERK_TH_F 8        /* doubles of one th_tab row */
#define D2D_JERK_TT_F 5        /* doubles of one tt_tab row */

#define D2D_JERK_STAT_TIE 1      /* the heading after the chosen one has the same cost and is free too: the tie decided */
#define D2D_JERK_STAT_UNKNOWN 2  /* the costs hold a tie and their weak order is not the table's: (cost, index) order was used */
#define D2D_JERK_STAT_SHIFT 8    /* stat >> 8: primitives the reference's lazy walk tests (rank of the choice + 1, or 72) */

typedef struct d2d_jerk_call {
  /* ---- the state's own buffers (include/d2d.h layouts) ---- */
  const double *drone;      /* [B][8] */
  const double *target;     /* [B][2] */
  const uint8_t *active;    /* [B][N]; may be NULL when N == 0 */
  const double *kf;         /* [B][N][20], mu first; may be NULL when N == 0 */
  const uint8_t *dmap;      /* [B][grid bytes] the explored map */
  /* ---- the library's per-env state ---- */
  double *trk_radius;       /* [B][N]; may be NULL when N == 0 */
  uint8_t *trk_prev;        /* [B][N]; may be NULL when N == 0 */
  /* ---- tables ---- */
  const double *th_tab;     /* [72][8] */
  const double *tt_tab;     /* [72][S][5] */
  const uint8_t *tie_perm;  /* [288][72] */
  const uint8_t *tie_eq;    /* [288][72] */
  /* ---- outputs ---- */
  uint8_t *plan_ok;         /* [B] */
  uint8_t *wp_valid;        /* [B] */
  double *wp;               /* [B][6] position, velocity, acceleration; zeros where wp_valid is 0 */
  int32_t *choice;          /* [B] heading index chosen, or -1 */
  int32_t *stat;            /* [B] D2D_JERK_STAT_* */
  /* ---- sizes and scalars ---- */
  int32_t B, N, S;
  int32_t W, H;             /* cells */
  int32_t grid_tile;        /* 0 (row-major [W][H]) or 16 */
  double scale;             /* params.map_scale */
  double W_px, H_px;        /* params.map_size */
  double drone_radius, agent_radius, var_cam;
  double half_v_max;        /* 0.5 * params.drone_max_speed, as the host multiplies it */
} d2d_jerk_call;

int d2d_jerk_version(void);
const char *d2d_jerk_last_error(void);

/* B >= 1, 0 <= N <= D2D_JERK_MAX_N, 1 <= S <= D2D_JERK_MAX_S (-4 above the limits), 1 <= W, H <= 32767, scale > 0.  Every `times`
 * of th_tab must lie in [1, S] (the device clamps what does not).  Every output entry of every env is written. */
int d2d_jerk_plan(const d2d_jerk_call *call, void *stream);

/* trk_radius <- trk_radius0 and trk_prev <- 0, [B][N] each, for every env (mask NULL) or the envs with mask[b * mask_stride] != 0 */
int d2d_jerk_reset(double *trk_radius, uint8_t *trk_prev, const double *trk_radius0, const uint8_t *mask, int32_t mask_stride, int32_t B,
                   int32_t N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_JERK_H */
