/*
 * d2d_rvo_live.h — the two launches of include/d2d_rvo.h for a batch in which some envs have finished their episode
 * (libd2d_rvo.so; VecDrone2DEnv.run_episodes with the Primitive plugins under motion_profile='RVO').
 *
 *   d2d_rvo_velocity_live     d2d_rvo_velocity for the envs that are not done; a finished env's vel_out is its vel
 *   d2d_rvo_agents_step_live  d2d_rvo_agents_step for the envs that are not done; a finished env's agents are not touched
 *
 * `flags` is the state's own d2d_state.flags, [B][4] bytes; byte D2D_RVO_LIVE_F_DONE of an env decides (D2D_F_DONE of include/d2d.h,
 * restated here so that this header stands alone).
 *
 * A live env gets bit for bit what the unmasked launch gives it.  The decision launch has one wave per (env, agent), so the test
 * is uniform over the wave: a finished env's wave builds no cone and takes no asin / atan2; it copies the agent's two entries of vel
 * to vel_out, so that the caller's swap of the two buffers keeps the velocity, and returns.  The move launch returns before it
 * reads anything of a finished env's agents.
 *
 * flags == NULL is refused with -1 (d2d_rvo_velocity / d2d_rvo_agents_step are the launches without a mask).  Sizes, error codes
 * and the thread-local message (d2d_rvo_last_error) are as in d2d_rvo.h.  The functions are additions to the library: its version
 * does not change with them, and a caller looks them up as optional symbols.
 */
#ifndef D2D_RVO_LIVE_H
#define D2D_RVO_LIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_RVO_LIVE_F_DONE 3 /* D2D_F_DONE of include/d2d.h: byte of flags[b][4] that says env b's episode has ended */

/* d2d_rvo_velocity with flags [B][4] (u8): every entry of vel_out is written, a finished env's with its entry of vel. */
int d2d_rvo_velocity_live(const double *agents, const double *vel, const int32_t *pillars, const uint8_t *flags, int32_t B, int32_t N,
                          int32_t P, double *vel_out, void *stream);

/* d2d_rvo_agents_step with flags [B][4] (u8): no row of a finished env's agents is written. */
int d2d_rvo_agents_step_live(double *agents, const double *vel, const uint8_t *flags, double W_px, double H_px, double scale, double dt,
                             int32_t B, int32_t N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_RVO_LIVE_H */
