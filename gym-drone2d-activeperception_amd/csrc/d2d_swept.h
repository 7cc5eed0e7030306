// include/d2d_swept.h: the swept-trajectory map replan_check returns (traj_planner.py:220-233) and its crop around the drone
// (envs/training_v3.py:206-209), one wave per env.  Included by d2d_hip.hip twice:
// behind its own kernels for the two kernels (they use sq_threshold, cell_fast, grid_ix, ld2 and d2d_lds of theirs), and with
// D2D_SWEPT_ENTRY_POINTS inside its extern "C" block for d2d_swept_mark / d2d_swept_crop (which use its fail, plan_check, fit_wpb).
//
// k_swept_mark holds the env's whole map in LDS (at most 256 x 256 bytes), next to the active trackers' (mu, lim).  The trajectory
// is walked in passes of 64 waypoints, lane = waypoint.  "Last write wins" has to hold across the lanes of a pass and across
// passes; a maximum over the stored value would do below 2560 waypoints, where trunc(i * dt) & 0xff wraps, so the order itself is
// kept instead: within a pass a lane whose cell a HIGHER lane of the pass also writes stays silent (63 lane reads of the cell
// index), so no two lanes of one LDS store name the same byte; and the LDS stores of one wave execute in order, so a later pass
// overwrites an earlier one.  A trajectory that leaves a cell and re-enters it is exact either way.  The finished plane goes out to
// the env's map whole, which is also what clears it.

#ifndef D2D_SWEPT_ENTRY_POINTS

// LDS of one wave of k_swept_mark: five planes of the active trackers (padded to four entries, as plan_env_quick walks them),
// then the map
__host__ __device__ inline size_t swept_trk_pad(int N) { return (size_t)((N + 3) & ~3); }
__host__ __device__ inline size_t swept_wave_bytes(const d2d_cfg &c) {
  return swept_trk_pad(c.N) * 5 * sizeof(double) + ((grid_bytes(c) + 15) & ~(size_t)15);
}

__global__ __launch_bounds__(WAVE *WAVES_PER_BLOCK) void k_swept_mark(d2d_cfg c, d2d_state s, d2d_plan p, d2d_swept w) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int e = blockIdx.x * (int)(blockDim.x / WAVE) + wv;
  if (e >= c.B) return;
  if (s.flags[(size_t)e * 4 + D2D_F_DONE] != 0) {  // a finished env keeps its map, crop and count (the contract of every _live launch)
    if (lane == 0) w.live[e] = 0;
    return;
  }
  const int N = c.N;
  const size_t NP = swept_trk_pad(N), gb = grid_bytes(c);
  char *base = d2d_lds + (size_t)wv * swept_wave_bytes(c);
  double *tmx = (double *)base, *tmy = tmx + NP, *tvx = tmy + NP, *tvy = tvx + NP, *tlim = tvy + NP;
  unsigned char *lm = (unsigned char *)(tlim + NP);
  uint32_t *lm32 = (uint32_t *)lm;
  const int ndw = (int)((gb + 3) >> 2);  // (the plane is padded to 16 bytes)
  for (int i = lane; i < ndw; i += WAVE) lm32[i] = 0u;
  const int hdr_l = p.traj_hdr[(size_t)e * 2 + (lane & 1)];
  // ---- the active trackers into LDS: plan_env_quick's compaction, READ-ONLY (the plan stage that follows does the bookkeeping).
  // A tracker that stage would reset (trk_prev && !active) is inactive and not tested, so the stored radius and limit are exact ----
  int nact = 0;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    bool act = false;
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, lim2 = 0;
    if (k < N) {
      const double *mu = s.kf + ((size_t)e * N + k) * D2D_KF;
      m0 = mu[0]; m1 = mu[1]; m2 = mu[2]; m3 = mu[3];
      act = s.active[(size_t)e * N + k] != 0;
      const double rad = p.trk_radius[(size_t)e * N + k];
      lim2 = p.trk_lim[(size_t)e * N + k];
      if (act && !(lim2 > 0.0)) lim2 = sq_threshold(c.drone_radius + rad);
    }
    const unsigned long long am = __ballot(act);
    if (act) {
      const int q = nact + __popcll(am & ((1ull << lane) - 1ull));
      tmx[q] = m0; tmy[q] = m1; tvx[q] = m2; tvy[q] = m3; tlim[q] = lim2;
    }
    nact += __popcll(am);
  }
  wave_sync_lds();
  // (a header outside the buffer cannot come from the plan stage; a caller's own is clipped to what can be read)
  const int head = max(__builtin_amdgcn_readlane(hdr_l, 0), 0);
  const int stored = min(__builtin_amdgcn_readlane(hdr_l, 1), p.traj_cap);
  const int n = max(stored - head, 0);
  const double *__restrict__ traj = p.traj + (size_t)e * p.traj_cap * 4;
  const double inv_scale = 1.0 / c.scale;
  int m = n;
  for (int i0 = 0; i0 < n; i0 += WAVE) {
    const int i = i0 + lane;
    const bool valid = i < n;
    bool hit = false;
    int cid = -1, sv = 0;
    if (valid) {
      const double2 wxy = ld2(traj + (size_t)(head + i) * 4);
      const double wx = wxy.x, wy = wxy.y;
      const double ti = (double)i * c.dt;
      const int ci = cell_fast(wx, c.scale, inv_scale), cj = cell_fast(wy, c.scale, inv_scale);
      if (ci >= 0 && ci < c.W && cj >= 0 && cj < c.H) cid = grid_ix(c, ci, cj);
      sv = ((int)ti) & 0xff;  // swep_map is uint8: the stored value is trunc(i * dt)
      for (int q = 0; q < nact; q += 4) {  // four trackers per round, loads first; the test is plan_env_quick's, operand for operand
        double mx[4], my[4], vx[4], vy[4], lim[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          mx[u] = tmx[q + u]; my[u] = tmy[q + u]; vx[u] = tvx[q + u]; vy[u] = tvy[q + u]; lim[u] = tlim[q + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double ex = mx[u] + ti * vx[u], ey = my[u] + ti * vy[u];
          const double dx = ex - wx, dy = ey - wy;
          hit = hit | ((q + u < nact) & (__builtin_fma(dy, dy, dx * dx) <= lim[u]));
        }
      }
    }
    // traj_planner.py:223-229 writes the cell before it tests the trackers and returns at the first hit: the hit waypoint is in the map
    const unsigned long long hb = __ballot(valid && hit);
    const int first = hb ? __ffsll((long long)hb) - 1 : WAVE - 1;
    if (hb) m = i0 + first + 1;
    const bool writes = valid && cid >= 0 && lane <= first;
    const int key = writes ? cid : -1 - lane;  // (a lane that writes nothing matches nobody)
    bool later = false;
    for (int j = 1; j < WAVE; ++j) later = later | ((j > lane) & (__builtin_amdgcn_readlane(key, j) == key));
    if (writes && !later) lm[cid] = (unsigned char)sv;
    if (hb) break;
  }
  wave_sync_lds();
  unsigned char *__restrict__ out = w.map + (size_t)e * gb;
  if ((gb & 3) == 0) {
    uint32_t *out32 = (uint32_t *)out;
    for (int i = lane; i < ndw; i += WAVE) out32[i] = lm32[i];
  } else {
    for (int i = lane; i < (int)gb; i += WAVE) out[i] = lm[i];
  }
  if (lane == 0) {
    w.count[e] = m;
    w.live[e] = 1;
  }
}

// The L x L zero-padded crop of the env's map around the drone's cell (its position after this step's control stage), lanes over
// the crop's bytes as st_obs maps them
__global__ __launch_bounds__(WAVE *WAVES_PER_BLOCK) void k_swept_crop(d2d_cfg c, d2d_state s, d2d_swept w) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int e = blockIdx.x * (int)(blockDim.x / WAVE) + wv;
  if (e >= c.B) return;
  if (w.live[e] == 0) return;
  const int L = c.L, edge = (L - 1) / 2, nn = L * L;
  const double inv_scale = 1.0 / c.scale;
  const double2 dpos = ld2(s.drone + (size_t)e * D2D_DF);
  const int i0 = cell_fast(dpos.x, c.scale, inv_scale) - edge, j0 = cell_fast(dpos.y, c.scale, inv_scale) - edge;
  const unsigned char *__restrict__ mp = w.map + (size_t)e * grid_bytes(c);
  unsigned char *__restrict__ ob = w.obs + (size_t)e * nn;
  for (int idx = lane; idx < nn; idx += WAVE) {
    const int pr = idx / L, q = idx - pr * L;
    const int i = i0 + pr, j = j0 + q;
    const bool in = i >= 0 && i < c.W && j >= 0 && j < c.H;
    ob[idx] = in ? mp[grid_ix(c, min(max(i, 0), c.W - 1), min(max(j, 0), c.H - 1))] : (unsigned char)0;
  }
}

#else

// ---- the entry points: the map replan_check returns, between the perceive and the plan launch, and its crop behind the act launch ----
static int swept_check(const d2d_cfg *c, const d2d_swept *w) {
  if (!w || !w->map || !w->obs || !w->count || !w->live) return fail(-1, "swept: null buffer");
  if (c->W > D2D_SWEPT_MAX_SIDE || c->H > D2D_SWEPT_MAX_SIDE) return fail(-4, "swept: maps of at most 256 x 256 cells");
  return 0;
}

int d2d_swept_mark(const d2d_cfg *c, const d2d_state *s, const d2d_plan *p, const d2d_swept *w, void *stream) {
  int rc = plan_check(c, s, p);
  if (rc) return rc;
  if ((rc = swept_check(c, w))) return rc;
  if (p->planner != D2D_PLAN_PRIMITIVE || p->traj_cap <= 0) return fail(-1, "swept: the map is the Primitive planner's (D2D_PLAN_PRIMITIVE)");
  if (c->N > 0 && (!s->kf || !s->active)) return fail(-1, "swept: null tracker buffers");
  const size_t wb = swept_wave_bytes(*c);
  if (wb > LDS_HARD) return fail(-4, "swept: too many agents for the tracker staging in LDS");
  if (c->B == 0) return 0;
  const int wpb = fit_wpb(wb);
  lds_optin(k_swept_mark, wb * wpb);
  hipLaunchKernelGGL(k_swept_mark, env_grid(c->B, wpb), env_block(wpb), wb * wpb, (hipStream_t)stream, *c, *s, *p, *w);
  return launched();
}

int d2d_swept_crop(const d2d_cfg *c, const d2d_state *s, const d2d_swept *w, void *stream) {
  int rc = check(c, s);
  if (rc) return rc;
  if ((rc = swept_check(c, w))) return rc;
  if (c->B == 0) return 0;
  hipLaunchKernelGGL(k_swept_crop, env_grid(c->B), env_block(), 0, (hipStream_t)stream, *c, *s, *w);
  return launched();
}

#endif
