/*
 * d2d_worlds_table.h — d2d_stream_assign for a stream whose episodes are the rows of a table (libd2d_worlds.so;
 * VecDrone2DEnv.stream_episodes(episodes=...), runner.EpisodeStream(episodes=...), runner.ValidationStudy).
 *
 * The stream of d2d_worlds_stream.h plays episode k in the world of map_id0 + k, and every episode shares one start position and one
 * target list.  The reference's validation study (script/validation_speed.py, validation_size.py, validation_shape.py) plays, per
 * cell, 5 maps x 72 (start, target) pairs: there episode k is row k of a table of (map id, env_par, env_tgt), the three per-env
 * inputs d2d_worlds_build_masked reads anyway.  Row k's env_par carries the start position, the number of targets, the radius range
 * and speed of the agents, and D2D_WE_REDRAW (include/d2d_worlds.h); its env_tgt the targets.
 *
 * What a table may vary: everything the world build reads per env.  What it may not: anything d2d_cfg, the planner tables or the
 * shapes of the batch are derived from -- the agent count, the agent radius where it moves the Kalman archive bounds (kf_lo_x ..),
 * drone_max_speed, the map.  Those are per stream, and the caller checks them (VecDrone2DEnv.stream_episodes names the field and
 * the row).
 *
 * d2d_stream_harvest, d2d_stream_clear, d2d_worlds_build_masked and the masked resets are used as they are.  An addition to the
 * library: D2D_WORLDS_VERSION does not change with it, and a caller looks it up as an optional symbol.  Error codes and the
 * thread-local message (d2d_worlds_last_error) are as in d2d_worlds.h.
 */
#ifndef D2D_WORLDS_TABLE_H
#define D2D_WORLDS_TABLE_H

#include <stdint.h>

#include "d2d_worlds_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup: d2d_stream_assign's scan, unchanged -- no atomics, the result is a function of the flags, slot_episode and counts
 * alone.  A slot e that receives episode k < M also copies that episode's row: map_id[e] = ep_map_id[k] ([M] uint32),
 * env_par[e] = ep_par[k] ([M][D2D_WORLDS_ENV_F] doubles), env_tgt[e] = ep_tgt[k] ([M][T][2] doubles).  env_par [B][D2D_WORLDS_ENV_F]
 * and env_tgt [B][T][2] are the arrays of the d2d_world_spec that d2d_worlds_build_masked reads next.  Retiring, cursor and finished
 * are d2d_stream_assign's; a slot that receives nothing keeps its map id and its rows.  The table pointers may be NULL for M == 0. */
int d2d_stream_assign_table(const uint8_t *flags, int32_t B, int64_t M, int32_t T, const uint32_t *ep_map_id, const double *ep_par,
                            const double *ep_tgt, int32_t *slot_episode, uint32_t *map_id, double *env_par, double *env_tgt,
                            uint8_t *refill, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_WORLDS_TABLE_H */
