/*
 * d2d_gaze.h — C ABI of the gaze decision of the step path (libd2d_gaze.so): what the reference's episode loop evaluates on the host
 * before every step, `a = policy.plan(policy, env.info)` (experiment.py:69), for every env of a batch in one launch.
 *
 *   d2d_gaze_act     one call per step, BEFORE the step (d2d_perceive / d2d_run_stages of include/d2d.h), on the state the previous
 *                    step left: writes action[B]
 *   d2d_gaze_reset   the Owl state of every env, or of the envs of a mask, back to all zero: Experiment.__init__ builds a fresh
 *                    policy per episode
 *
 * Kinds
 *   D2D_GAZE_K_LOOKAHEAD  yaw_planner.py:28-39.  Zero velocity: 0.  Else heading = math.degrees(math.atan2(-vy, vx)) % 360, the yaw
 *                         rate max(min((heading - yaw) / dt, w), -w) with Python's min / max, its sign flipped unless
 *                         abs(heading - yaw) < 180, divided by w = drone_max_yaw_speed.  One lane per env.
 *   D2D_GAZE_K_OWL        yaw_planner.py:151-222, operation for operation (csrc/gaze/d2d_gaze.h holds the arithmetic): the held
 *                         decision (`self.u`), update_U over the 36 directions, d_g, d_v, d_o, G, U, the five-term
 *                         f[i, :].dot(lamb) as a chain of FMAs from 0, `** 2` as libm's pow(x, 2.0), np.argmin (the first minimum,
 *                         the first NaN wins), and the zip(d_o, trackers) pairing: the j-th ACTIVE tracker's direction with tracker
 *                         j's state.  A drone at rest makes every cost NaN and the policy picks candidate 0; nothing special-cases
 *                         it.  One wave per env; an env that only pops its held decision (owl_tab[D2D_OWL_T_HOLD] of every
 *                         D2D_OWL_T_HOLD + 1 calls) reads its flag and two doubles and writes two: no tracker walk, no atan2.
 *
 * The Owl state and table have the layouts include/d2d.h defines for the Owl stage of libd2d_hip.so, restated here so that this
 * header stands alone: owl_state [B][D2D_GAZE_OWL_STATE_F] = the 36 scores, the held rate (deg / s) at D2D_GAZE_OWL_S_RATE, the calls
 * left that repeat it at D2D_GAZE_OWL_S_LEFT; owl_tab [D2D_GAZE_OWL_TAB_LEN] = D2D_OWL_T_* of include/d2d.h (the host builds it with
 * the reference's own expressions).
 *
 * Finished envs.  With `flags` given, an env whose flags[D2D_F_DONE] (byte 3 of its four) is set is left untouched: its action, its
 * scores, its held rate and count.  The reference's loop does not call the policy after `done`.
 *
 * Conventions as in d2d_jerk.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 bad argument, -3 HIP launch error, -4 unsupported size) with a thread-local message and no launch.  The library
 * is separate from libd2d_hip.so and reports its own version.
 */
#ifndef D2D_GAZE_H
#define D2D_GAZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_GAZE_VERSION 1

#define D2D_GAZE_K_LOOKAHEAD 2 /* the numbers of D2D_GAZE_LOOKAHEAD / D2D_GAZE_OWL of include/d2d.h */
#define D2D_GAZE_K_OWL 5
#define D2D_GAZE_MAX_N 1024 /* trackers of one env */
#define D2D_GAZE_OWL_STATE_F 40
#define D2D_GAZE_OWL_S_RATE 36
#define D2D_GAZE_OWL_S_LEFT 37
#define D2D_GAZE_OWL_TAB_LEN 160

typedef struct d2d_gaze_call {
  /* ---- the state's own buffers (include/d2d.h layouts) ---- */
  const double *drone;   /* [B][8] */
  const double *target;  /* [B][2]; Owl */
  const uint8_t *active; /* [B][N]; Owl; may be NULL when N == 0 */
  const double *kf;      /* [B][N][20], mu first; Owl; may be NULL when N == 0 */
  const uint8_t *flags;  /* [B][4], or NULL: every env decides */
  /* ---- the library's per-env state and the host's table ---- */
  double *owl_state;     /* [B][D2D_GAZE_OWL_STATE_F]; Owl */
  const double *owl_tab; /* [D2D_GAZE_OWL_TAB_LEN]; Owl */
  /* ---- output ---- */
  double *action;        /* [B] */
  /* ---- sizes and scalars ---- */
  int32_t B, N;
  int32_t kind;          /* D2D_GAZE_K_* */
  int32_t reserved;      /* 0 */
  double dt;             /* params.dt */
  double yaw_rate_max;   /* params.drone_max_yaw_speed */
} d2d_gaze_call;

int d2d_gaze_version(void);
const char *d2d_gaze_last_error(void);

/* B >= 1, 0 <= N <= D2D_GAZE_MAX_N (-4 above), kind one of D2D_GAZE_K_* (-1 otherwise), dt > 0, yaw_rate_max > 0.  LookAhead reads
 * drone and flags alone. */
int d2d_gaze_act(const d2d_gaze_call *call, void *stream);

/* owl_state [B][D2D_GAZE_OWL_STATE_F] <- 0 for every env (mask NULL) or the envs with mask[b * mask_stride] != 0 */
int d2d_gaze_reset(double *owl_state, const uint8_t *mask, int32_t mask_stride, int32_t B, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_GAZE_H */
