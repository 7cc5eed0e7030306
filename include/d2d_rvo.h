/*
 * d2d_rvo.h — C ABI of the RVO motion profile on the device (libd2d_rvo.so): the reference's `--motion_profile RVO`, in which every
 * agent picks, once per step, a velocity outside the reciprocal velocity obstacles of the other agents and the velocity obstacles
 * of the pillars, and then moves with it (envs/drone_v2.py:169-175).
 *
 *   d2d_rvo_velocity     utils.py:299-460   RVO.RVO_update, intersect, in_between: the decision of every agent    -> vel_out
 *   d2d_rvo_agents_step  utils.py:472-493   Agent.step with `velocity` and `pref_velocity` as separate arrays     -> agents
 *
 * Two launches per step, because no agent may move while another agent's decision still reads its position: RVO_update captures
 * every agent's position and velocity before its loop (utils.py:304-306) and `agents[i].velocity = ...` (:356) rebinds, so the
 * captured lists keep the arrays of before the call.  All N decisions of an env are independent.
 *
 * What the decision reproduces, bit for bit (csrc/rvo/d2d_rvo.h holds the arithmetic):
 *   :308        ROB_RAD = agents[0].radius + 0.01, for every agent of the env
 *   :315-333    one cone per other agent: apex pA + 0.5 * (vB + vA), dist = norm(pA - pB) raised to 2 * ROB_RAD where below it,
 *               half angle asin(2 * ROB_RAD / dist), bounds cos / sin of theta_BA +- half
 *   :334-352    one cone per pillar (x, y, r): apex pA, radius r * 1.5 + ROB_RAD, the same clamp
 *   :366-393    the candidates: theta over np.arange(0, 2 * 3.14, 0.2) (32 values), rad over np.arange(0.02, |pref| + 0.02,
 *               |pref| / 5.0) by numpy's own length and fill rule (5 values for almost every speed, 6 for a few), theta-major,
 *               then pref itself: 161 or 193 candidates.  A candidate is unsuitable if in_between holds for ANY cone (the `break`
 *               at :376 only saves time); atan2 of the cone's bounds (:372-373) is a constant of the cone
 *   :395-397    some candidate suitable: Python's min(suitable_V, key=norm(v - pref)), the first minimum in list order
 *   :403-431    none suitable: tc per candidate = Python's min over the cones it lies in of dist_tg / norm(dif); the key
 *               0.2 / (tc + 0.001) + norm(v - pref), first minimum in list order.  A candidate exactly on an apex (dif == 0; two
 *               cell agents of one group, whose apex is pA + pref, reach it) divides by norm(dif) = 0 under the reference's
 *               np.seterr.  With finite inputs that is always a positive dist_tg over 0, an infinity: 0 / 0 needs dist_tg == 0, which
 *               needs a clamped cone, and in_between's 3.14 keeps theta_dif = atan2(0, 0) = 0 out of a cone that is pi wide.  The
 *               parallel argmin still returns what the sequential min returns for a NaN key (it wins only as the first element of
 *               the list, a later one never does): two compares, held to Python's min on lists by tests/test_rvo_model_cpu.py
 *
 * RVO_update returning False (:353-354, the env then reports done): its `try` covers only the cone set-up, where after the clamps
 * dist > 0 and the asin argument lies in (0, 1], so neither math.asin nor a division can raise.  There is no such path here.
 * len(agents) == 0 runs nothing (drone_v2.py:170): N == 0 is accepted and launches nothing.  N == 1 with P == 0 has no cone and takes
 * pref.  A preferred speed of exactly 0 makes np.arange raise outside the `try`; callers refuse agent_max_speed == 0 (and
 * agent_radius == -1 is refused with it: VecDrone2DEnv), the device then takes pref as the only candidate.
 *
 * Shape of d2d_rvo_velocity: one wave per (env, agent).  Its lanes first build the env's N - 1 + P cones of that agent into LDS
 * (six doubles each), then take the candidates 64 at a time (193 = 3 * 64 + 1: the fourth pass holds one lane) against every cone,
 * then reduce (key, index) over the wave.  LDS holds at most D2D_RVO_MAX_CONES = 1024 cones (48 KB of the 64 KB a workgroup may
 * ask for): N - 1 + P above that is refused with -4 rather than split.  BASELINE config 3 has 172 agents.
 *
 * Conventions as in d2d_metrics.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 bad argument, -3 HIP launch error, -4 unsupported size) with a thread-local message.  The library is separate
 * from libd2d_hip.so and reports its own version; no struct of d2d.h is involved: `agents` is the state's own d2d_state.agents,
 * [B][6][N] doubles (rows D2D_A_PX, PY, VX, VY, R, R2), whose rows VX, VY hold pref_velocity.
 */
#ifndef D2D_RVO_H
#define D2D_RVO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_RVO_VERSION 1

#define D2D_RVO_MAX_CONES 1024       /* N - 1 + P of one env: the cones one wave keeps in LDS */
#define D2D_RVO_MAX_ELEMS 0x7fffffff /* B * N, the waves of one call; B * 6 * N, the doubles of `agents` */

int d2d_rvo_version(void);
const char *d2d_rvo_last_error(void);

/* agents [B][6][N] (rows PX, PY; VX, VY = pref_velocity; R: row R's entry 0 gives ROB_RAD), vel [B][2][N] (agent.velocity: x row,
 * y row), pillars [B][P][3] (i32: x, y, r; may be NULL when P == 0) -> vel_out [B][2][N], the velocity RVO_update assigns to every
 * agent.  vel_out must not overlap vel or agents; neither input is modified.  Every entry of vel_out is written whatever the buffer
 * held.  B >= 1, N >= 0, P >= 0 (N == 0: nothing to do, 0 is returned); N - 1 + P <= D2D_RVO_MAX_CONES and B * 6 * N <=
 * D2D_RVO_MAX_ELEMS (-4 otherwise). */
int d2d_rvo_velocity(const double *agents, const double *vel, const int32_t *pillars, int32_t B, int32_t N, int32_t P, double *vel_out,
                     void *stream);

/* Agent.step of every agent, moving with vel [B][2][N] (what d2d_rvo_velocity wrote): position += vel * dt; pref_velocity is rotated
 * by 30 degrees where norm(vel) <= 5 and flipped at the map's border; both are written back into agents (rows PX, PY, VX, VY; rows R,
 * R2 are not touched).  W_px, H_px, scale, dt: params.map_size, map_scale, dt.  Sizes as d2d_rvo_velocity. */
int d2d_rvo_agents_step(double *agents, const double *vel, double W_px, double H_px, double scale, double dt, int32_t B, int32_t N,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_RVO_H */
