/*
 * d2d_worlds.h — C ABI of the world construction on the device (libd2d_worlds.so).
 *
 * Replaces, for a whole batch at once, what the reference's Drone2DEnv2.__init__ does before the first step:
 * envs/drone_v2.py:79-80 (random.seed(map_id), np.random.seed(map_id)), :13-66 (`init_obstacles_random_size`: pillars by
 * rejection, agents by rejection, one radius-5 agent per cell of the static map), :46 / utils.py:184 (tracker radii),
 * utils.py:495-525 (`OccupancyGridMap.init_obstacles`: border, pillar discs, agent discs), utils.py:718 (start yaw),
 * traj_planner.py:22 (planner target) and utils.py:181 (Kalman defaults).  The package's host_init.init_world is the same
 * construction in Python, one env at a time; this library fills the same fields with the same bits.
 *
 * Conventions as in d2d.h: plain C, the caller owns all memory, DEVICE pointers, asynchronous on the caller's stream, 0 or a
 * negative error (-1 bad argument, -2 version mismatch, -3 HIP launch error, -4 unsupported configuration) with a thread-local
 * message.  The library is separate from libd2d_hip.so (it shares no kernel with the step) and reports its own version; no
 * struct of d2d.h changes.
 */
#ifndef D2D_WORLDS_H
#define D2D_WORLDS_H

#include <stdint.h>

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_WORLDS_VERSION 1

#define D2D_WORLDS_ENV_F 8 /* doubles per env of d2d_world_spec.env_par */
#define D2D_WE_R_LO 0      /* uniform(a, b) of the radius (drone_v2.py:31-34): a ...                          */
#define D2D_WE_R_W 1       /* ... and b - a: (5, 10) for agent_radius == -1, else (agent_radius - 2, 4)       */
#define D2D_WE_SPEED 2     /* agent_max_speed                                                                 */
#define D2D_WE_TRK_R 3     /* float(agent_radius): tracker radius of the static-map agents (utils.py:184)     */
#define D2D_WE_X0 4        /* init_position                                                                   */
#define D2D_WE_Y0 5
#define D2D_WE_NTGT 6      /* len(target_list) <= T                                                           */
#define D2D_WE_REDRAW 7    /* 0: the world as constructed.  Non-zero: the world of script/validation_speed.py:134-138 -- after the
                              last agent is placed the env's Python `random` stream goes on, and every agent in agent order, the
                              static map's cell agents included, gets the preferred velocity (agents[A_VX], agents[A_VY])
                              vel * (cos, sin)(angle) with vel = random() * 40 + 20, angle = random() * 2 * pi.  Nothing else of
                              the env changes: the numpy stream (d2d_state.rng) is not touched                  */

#define D2D_WORLDS_MAX_ATTEMPTS 65536 /* default of d2d_world_spec.max_attempts */

/* status word of an env */
#define D2D_WORLD_OK 0
#define D2D_WORLD_CAP 1 /* max_attempts reached before every pillar and agent was placed (the reference would loop for ever):
                           every field of the env is 0 */

typedef struct d2d_world_spec {
  int32_t version;      /* D2D_WORLDS_VERSION */
  int32_t B;            /* worlds to build: env e of every array below */
  int32_t N;            /* agents per env = n_rand + n_cells */
  int32_t n_rand;       /* agent_number: placed by rejection (drone_v2.py:28-47) */
  int32_t n_cells;      /* non-zero cells of the static map (drone_v2.py:49-66) */
  int32_t P;            /* pillar_number (drone_v2.py:14-26) */
  int32_t T;            /* rows of targets per env (>= 1) */
  int32_t W_px, H_px;   /* map_size */
  int32_t scale;        /* map_scale */
  int32_t W, H;         /* W_px // scale, H_px // scale */
  int32_t grid_tile;    /* d2d_cfg.grid_tile: 0 or 16 */
  int32_t max_attempts; /* cap on pillar attempts + agent attempts + randint redraws of one env */
  double start_clear;   /* drone_radius + 70 (drone_v2.py:22, :43) */
  double pillar_clear;  /* drone_radius + 20 (drone_v2.py:19) */
  /* per batch */
  const double *unit;     /* [n_rand][2] (cos, sin)(2 pi k / n_rand) as the host's numpy evaluates them (drone_v2.py:35) */
  const int32_t *cells;   /* [n_cells][3] (x, y, label) of the static map's non-zero cells, x-major; 0 < label < 100 */
  /* per env */
  const uint32_t *map_id; /* [B] */
  const double *env_par;  /* [B][D2D_WORLDS_ENV_F] */
  const double *env_tgt;  /* [B][T][2] target_list, rows from len(target_list) on are 0 */
  /* outputs beside the state */
  double *tracker_radius; /* [B][N] drone.trackers[k].radius */
  int32_t *obstacles;     /* [B][P][3] the pillars (x, y, radius) */
  int32_t *status;        /* [B] D2D_WORLD_* */
} d2d_world_spec;

int d2d_worlds_version(void);
const char *d2d_worlds_last_error(void);

/* Fills, for env e < spec->B, the world fields of `st` (agents, agent_unit, dyn_prev, gt, dmap, drone, target, targets, counters,
 * active, kf and kf_len unless NULL, rng unless NULL: key after its first regeneration, position 200) and the three outputs of
 * `spec`.  The other fields of `st` are not read.  One wave per env; every loop is bounded by max_attempts or by the sizes of
 * `spec`, so the call returns whatever the parameters are. */
int d2d_worlds_build(const d2d_world_spec *spec, const d2d_state *st, void *stream);

/* (waves per workgroup, dynamic LDS bytes per workgroup) of the launch d2d_worlds_build would make; needs no GPU */
int d2d_worlds_launch_shape(const d2d_world_spec *spec, int32_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* D2D_WORLDS_H */
