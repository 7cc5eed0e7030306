// d2d_jerk_wave.inc -- the body of jerk_plan_kernel (one wave = one workgroup = env blockIdx.x of the call `c`), shared as text with
// jerk_plan_live_kernel, which tests the env's done byte first (include/d2d_jerk_live.h): jerk_plan_kernel compiles to what it always did.
  extern __shared__ __attribute__((aligned(16))) double trk[];   // [5][cap]
  __shared__ double cost[NT];
  __shared__ int order[NT];
  __shared__ int seen[NT];
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  const int N = c.N, cap = N > 0 ? N : 1, S = c.S;

  // ---- trackers: archive bookkeeping (utils.py:184, 238) and the active ones into LDS ----
  int na = 0;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    bool act = false;
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, rad = 0;
    if (k < N) {
      const size_t ik = b * N + k;
      const double *mu = c.kf + ik * D2D_JERK_KF;
      m0 = mu[0]; m1 = mu[1]; m2 = mu[2]; m3 = mu[3];
      act = c.active[ik] != 0;
      const bool prev = c.trk_prev[ik] != 0;
      rad = c.trk_radius[ik];
      if (prev && !act) {
        rad = c.agent_radius;
        c.trk_radius[ik] = rad;
      }
      if (prev != act) c.trk_prev[ik] = act ? 1 : 0;
    }
    const unsigned long long am = __ballot(act);
    if (act) {
      const int q = na + __popcll(am & ((1ull << lane) - 1ull));   // q < N <= cap
      trk[q] = m0; trk[cap + q] = m1; trk[2 * cap + q] = m2; trk[3 * cap + q] = m3;
      trk[4 * cap + q] = c.drone_radius + rad + 5.0 + c.var_cam;
    }
    na += __popcll(am);
  }

  const double *dr = c.drone + b * D2D_JERK_DF;
  d2d_jerk_env e = {{dr[0], dr[1]}, {dr[3], dr[4]}, {dr[5], dr[6]}, {c.target[2 * b], c.target[2 * b + 1]},
                    c.dmap + b * d2d_jerk_grid_bytes(c.W, c.H, c.grid_tile), trk, cap, na, 1.0 / c.scale, c.drone_radius + 10.0};

  // ---- costs, ranks by (cost, index), the tie table ----
  const double pm = d2d_jerk_mod360(d2d_jerk_phi(e.p0[0], e.p0[1], e.g[0], e.g[1]));
  for (int i = lane; i < NT; i += WAVE) {
    cost[i] = d2d_jerk_cost(i, pm);
    order[i] = i;
    seen[i] = 0;
  }
  __syncthreads();
  if (pm == pm) {
    int rank[2] = {0, 0};
    for (int u = 0, i = lane; i < NT; i += WAVE, ++u) {
      const double ci = cost[i];
      int r = 0;
      for (int j = 0; j < NT; ++j) {
        const double cj = cost[j];
        r += (cj < ci || (cj == ci && j < i)) ? 1 : 0;
      }
      rank[u] = r;                                     // a permutation of 0 .. 71: the costs are not NaN
    }
    __syncthreads();
    for (int u = 0, i = lane; i < NT; i += WAVE, ++u) order[rank[u]] = i;
  }
  __syncthreads();
  const int pat = d2d_jerk_pattern(pm);
  const uint8_t *perm = c.tie_perm + (size_t)pat * NT, *eq = c.tie_eq + (size_t)pat * NT;
  bool fits = true, tied = false;
  for (int r = lane; r < NT; r += WAVE) {
    const int t0 = perm[r], t1 = r + 1 < NT ? perm[r + 1] : 0;
    if (t0 >= NT || t1 >= NT) {
      fits = false;
    } else {
      atomicAdd(&seen[t0], 1);
      if (r + 1 < NT) {
        const double x = cost[t0], y = cost[t1];
        if (!(eq[r] ? x == y : x < y)) fits = false;
      }
    }
    if (r + 1 < NT) tied = tied || cost[order[r]] == cost[order[r + 1]];
  }
  __syncthreads();
  for (int r = lane; r < NT; r += WAVE) fits = fits && seen[r] == 1;
  const bool use_table = __ballot(!fits) == 0ull;
  int stat = 0;
  if (!use_table && (__ballot(tied) != 0ull || pm != pm)) stat |= D2D_JERK_STAT_UNKNOWN;
  __syncthreads();
  if (use_table)
    for (int r = lane; r < NT; r += WAVE) order[r] = perm[r];
  __syncthreads();

  // ---- the walk ----
  int found = -1;
  if (S <= WAVE) {
    const int per = WAVE / S, q = lane / S, s = lane - q * S;
    const unsigned long long ones = S == WAVE ? ~0ull : (1ull << S) - 1ull;
    for (int r0 = 0; r0 < NT && found < 0; r0 += per) {
      const int r = r0 + q;
      bool bad = false;
      if (q < per && r < NT) {
        const int th = order[r];
        if (s < d2d_jerk_times(&c, th)) {
          d2d_jerk_prim pr;
          d2d_jerk_primitive(c.th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c.half_v_max, &pr);
          bad = !d2d_jerk_sample_free(&c, &e, &pr, th, s);
        }
      }
      const unsigned long long bm = __ballot(bad);
      for (int u = 0; u < per && r0 + u < NT; ++u)
        if (((bm >> (u * S)) & ones) == 0ull) {
          found = r0 + u;
          break;
        }
    }
  } else {
    for (int r = 0; r < NT && found < 0; ++r)
      if (prim_free(c, e, order[r], lane)) found = r;
  }
  const int th = found >= 0 ? order[found] : -1;
  if (found >= 0 && found + 1 < NT && cost[order[found + 1]] == cost[th] && prim_free(c, e, order[found + 1], lane))
    stat |= D2D_JERK_STAT_TIE;

  if (lane == 0) {
    double *wp = c.wp + b * 6;
    if (found >= 0) {
      const double *tt = c.tt_tab + (size_t)th * S * D2D_JERK_TT_F;
      d2d_jerk_prim pr;
      d2d_jerk_primitive(c.th_tab + (size_t)th * D2D_JERK_TH_F, e.p0, e.v0, e.a0, e.g, c.half_v_max, &pr);
      for (int ii = 0; ii < 2; ++ii) {
        wp[ii] = d2d_jerk_pos(&pr, ii, tt, e.p0[ii], e.v0[ii], e.a0[ii]);
        wp[2 + ii] = d2d_jerk_vel(&pr, ii, tt, e.v0[ii], e.a0[ii]);
        wp[4 + ii] = d2d_jerk_acc(&pr, ii, tt, e.a0[ii]);
      }
    } else {
      for (int i = 0; i < 6; ++i) wp[i] = 0.0;
    }
    c.choice[b] = th;
    c.plan_ok[b] = c.wp_valid[b] = found >= 0 ? 1 : 0;
    c.stat[b] = stat | ((found >= 0 ? found + 1 : NT) << D2D_JERK_STAT_SHIFT);
  }
