// d2d_plan_spec.h -- the two sets of values the specialised kernels fold into constants, each as a pair of functions: `matches`
// (host: does this configuration hold exactly those values?) and `apply` (device: overwrite the kernel's own copy with the literals the
// host has verified, so that the compiler sees immediates where it saw loaded scalars).
//   * the reference's default geometry (utils.py:66-72), d2d_cfg: spec_default_matches / spec_default_apply;
//   * the plugins' parameters at that geometry as the reference's Params hand them to Primitive and Oxford, d2d_plan:
//     plan_default_matches / plan_default_apply -- the persistent kernel k_closed<1, true> (d2d_hip.hip).
// Every double is compared as a value with `==` against the literal that `apply` writes: a plan that matches is left bit-identical in
// the fields `apply` touches (tests/test_plan_spec_cpu.py compiles this header for the host and checks both).
// Pointers, capacities (traj_cap, node_cap, hash_cap), the pairwise plan's sizes, tobs_len and the arccos window stay run-time values.
#ifndef D2D_PLAN_SPEC_H
#define D2D_PLAN_SPEC_H

#include "../../include/d2d.h"

#if defined(__HIPCC__)
#define D2D_SPEC_HD __host__ __device__ inline
#define D2D_SPEC_D __device__ __forceinline__
#define D2D_SPEC_CONSTEXPR __host__ __device__ constexpr
#else  // a plain host build (the CPU tests)
#define D2D_SPEC_HD static inline
#define D2D_SPEC_D static inline
#define D2D_SPEC_CONSTEXPR constexpr
#endif

// SPEC 1: N <= 16 agent slots, SPEC 2: N <= 40 (the default map plus the 14 obstacle_map agents, the reference's sweeps of up
// to 30 agents; 40 is where both grids whole + the agent planes still leave four workgroups per CU in every phase), SPEC 3: the
// default geometry with any N (LDS capacity and waves per workgroup stay run-time values)
D2D_SPEC_CONSTEXPR int spec_ncap(int spec) { return spec == 1 ? 16 : (spec == 2 ? 40 : 0); }

D2D_SPEC_HD bool spec_default_matches(const d2d_cfg &c) {
  return c.W == 50 && c.H == 50 && c.R == 50 && c.L == 33 && c.dt == 0.1 && c.scale == 10.0 &&
         c.W_px == 500.0 && c.H_px == 500.0 && c.ray_off0 == -0x1.921fb54442d18p-1 && c.ray_dth == 0x1.015bf9217271ap-5 &&
         c.depth == 80.0 && c.drone_radius == 10.0 && c.yaw_rate == 80.0 && c.max_acc == 40.0 && c.max_steps == 800.0 &&
         c.sigma == 0.0 && c.grid_tile == 0;
}

D2D_SPEC_D void spec_default_apply(d2d_cfg &c) {
  c.W = 50; c.H = 50; c.R = 50; c.L = 33;
  c.dt = 0.1; c.scale = 10.0; c.W_px = 500.0; c.H_px = 500.0;
  c.ray_off0 = -0x1.921fb54442d18p-1; c.ray_dth = 0x1.015bf9217271ap-5;
  c.depth = 80.0; c.drone_radius = 10.0; c.yaw_rate = 80.0; c.max_acc = 40.0; c.max_steps = 800.0; c.sigma = 0.0;
  c.grid_tile = 0;
}

// The plugins' parameters of the headline workload (README's command; BASELINE.json configs[1]): Primitive + Oxford on the default
// geometry with at most 16 agents, and what Params' defaults give their constructors (device_plugins.build_tables) --
//   u_space = arange(-40, 40, 11): nu = 8, an expansion is one batch of 64 primitives; sample_num = 40 * 2 // 10 = 8;
//   np.arange(2, 0, -0.1): n_ts = 20; max_itr = 100; horizon 2; drone_max_speed 40; safe_dist = drone_radius + 10 = 20; threshold 10;
//   v_yaw_space = arange(-80, 80, 80 / 3): n_yaw = 6; drone_max_yaw_speed 80; half_fov = math.radians(90 / 2);
//   vmax_sq / goal_sq: the NON-ZERO thresholds of 40 and 10 (d2d.h: the largest s with sqrt(s) < 40, with sqrt(s) <= 10);
//   agent_radius 15, that workload's (a tracker's radius after an archive, utils.py:184).
D2D_SPEC_HD bool plan_default_matches(const d2d_cfg &c, const d2d_plan &p) {
  return spec_default_matches(c) && c.N <= spec_ncap(1) &&  // (the instantiation SPEC 1 only)
         p.planner == D2D_PLAN_PRIMITIVE && p.gaze == D2D_GAZE_OXFORD &&
         p.nu == 8 && p.n_sample == 8 && p.n_ts == 20 && p.max_itr == 100 && p.n_yaw == 6 &&
         p.horizon == 2.0 && p.vmax == 40.0 && p.safe_dist == 20.0 && p.goal_tol == 10.0 && p.agent_radius == 15.0 &&
         p.half_fov == 0x1.921fb54442d18p-1 && p.yaw_rate_max == 80.0 &&
         p.vmax_sq == 0x1.8fffffffffffep+10 && p.goal_sq == 0x1.9000000000001p+6;
}

D2D_SPEC_D void plan_default_apply(d2d_plan &p) {
  p.planner = D2D_PLAN_PRIMITIVE; p.gaze = D2D_GAZE_OXFORD;
  p.nu = 8; p.n_sample = 8; p.n_ts = 20; p.max_itr = 100; p.n_yaw = 6;
  p.horizon = 2.0; p.vmax = 40.0; p.safe_dist = 20.0; p.goal_tol = 10.0; p.agent_radius = 15.0;
  p.half_fov = 0x1.921fb54442d18p-1; p.yaw_rate_max = 80.0;
  p.vmax_sq = 0x1.8fffffffffffep+10; p.goal_sq = 0x1.9000000000001p+6;
}

#endif
