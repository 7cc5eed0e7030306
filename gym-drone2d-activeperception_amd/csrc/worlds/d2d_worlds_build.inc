// d2d_worlds_build.inc — the body of worlds_build_kernel, shared as text with worlds_build_masked_kernel (d2d_worlds.hip): one wave
// builds env e = blockIdx.x of spec `s` into state `st`; `ok` says at the end whether the world was placed within max_attempts.
  extern __shared__ double lds[];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int N = s.N, nr = s.n_rand, P = s.P, T = s.T, W = s.W, H = s.H, tile = s.grid_tile, cap = s.max_attempts;
  double *acc = lds;                                  // [nr][D2D_W_ACC_F]
  uint32_t *buf = (uint32_t *)(acc + (size_t)D2D_W_ACC_F * nr);   // [D2D_W_BUF]
  int32_t *pil = (int32_t *)(buf + D2D_W_BUF);        // [P][3]
  uint32_t *key = buf + D2D_W_CARRY;
  const double *par = s.env_par + (size_t)e * D2D_WORLDS_ENV_F, *tgt = s.env_tgt + (size_t)e * T * 2;
  const uint32_t seed = s.map_id[e];
  const double scale = (double)s.scale;

  // ---- the Python stream: pillars, then agents
  if (lane == 0) d2d_w_seed_python(key, seed);
  __syncthreads();
  int p = D2D_W_BUF, attempts = 0, ok = 1;

  const uint32_t pn[3] = {(uint32_t)(s.W_px - 99), (uint32_t)(s.H_px - 99), 6u};
  const int plo[3] = {50, 50, 15};
  int np_ = 0;
  for (int it = 0; it < cap && ok && np_ < P; ++it) {   // every round takes at least one attempt
    if (attempts >= cap) { ok = 0; break; }
    attempts += 1;
    int v[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int k = d2d_w_bit_length(pn[c]);
      int got = 0;
      for (int rd = 0; rd < cap && ok; ++rd) {          // every redraw counts as an attempt
        stream_ensure(buf, p, 1, lane);
        const uint32_t r = d2d_rng_temper(buf[p++]) >> (32 - k);
        if (r < pn[c]) { v[c] = plo[c] + (int)r; got = 1; break; }
        if (++attempts >= cap) ok = 0;
      }
      if (!got) ok = 0;
    }
    if (!ok) break;
    if (d2d_w_pillar_free(v[0], v[1], v[2], par, tgt, s.pillar_clear, s.start_clear)) {
      __syncthreads();
      if (lane < 3) pil[3 * np_ + lane] = lane == 0 ? v[0] : lane == 1 ? v[1] : v[2];
      __syncthreads();
      np_ += 1;
    }
  }
  if (np_ < P) ok = 0;

  int na = 0;
  const double xw = (double)(s.W_px - 20 - 20), yw = (double)(s.H_px - 20 - 20);
  for (int pass = 0; pass < cap && ok && na < nr; ++pass) {   // every pass takes at least one attempt
    if (attempts >= cap) { ok = 0; break; }
    stream_ensure(buf, p, 6, lane);
    const int n = min(min((D2D_W_BUF - p) / 6, WAVE), cap - attempts);
    double x = 0.0, y = 0.0, r = 0.0;
    bool free_ = false;
    if (lane < n) {
      const uint32_t *g = buf + p + 6 * lane;
      x = d2d_w_uniform(20.0, xw, d2d_rng_temper(g[0]), d2d_rng_temper(g[1]));
      y = d2d_w_uniform(20.0, yw, d2d_rng_temper(g[2]), d2d_rng_temper(g[3]));
      r = d2d_w_uniform(par[D2D_WE_R_LO], par[D2D_WE_R_W], d2d_rng_temper(g[4]), d2d_rng_temper(g[5]));
      free_ = d2d_w_agent_free_static(x, y, r, par, P, pil, s.start_clear) != 0;
      for (int q = 0; q < na; ++q)
        if (d2d_w_norm(acc[4 * q] - x, acc[4 * q + 1] - y) <= acc[4 * q + 2] + r) free_ = false;
    }
    int used = n, lo = 0;
    for (int round = 0; round < WAVE; ++round) {        // the free lanes in order: each accepted one is tested by those behind it
      const unsigned long long m = __ballot(free_ && lane >= lo);
      if (m == 0ull) break;
      const int f = __ffsll((long long)m) - 1;
      const double fx = shfl_f64(x, f), fy = shfl_f64(y, f), fr = shfl_f64(r, f);
      if (lane == f) {
        acc[4 * na] = x;
        acc[4 * na + 1] = y;
        acc[4 * na + 2] = r;
      }
      na += 1;
      if (na == nr) { used = f + 1; break; }            // the words behind the attempt that completes the list stay undrawn
      lo = f + 1;
      if (free_ && lane > f && d2d_w_norm(fx - x, fy - y) <= fr + r) free_ = false;
    }
    __syncthreads();                                    // the accepted list, for the next pass
    attempts += used;
    p += 6 * used;
  }
  if (na < nr) ok = 0;

  // ---- the redraw (D2D_WE_REDRAW): the stream goes on behind the last agent, four words per agent and none depends on another, so
  // lane j takes agent k0 + j of a pass.  A pass ends at the key's end: what is left of it (fewer than four words) moves into the
  // carry and the key is regenerated, as for the attempts.  The velocities go straight to the agent records, which the record
  // loop below then leaves alone: the key is about to make room for numpy's, and no LDS is spent on them.
  const bool redraw = ok && par[D2D_WE_REDRAW] != 0.0;
  if (redraw) {
    double *avx = st.agents + ((size_t)e * D2D_AF + D2D_A_VX) * N, *avy = st.agents + ((size_t)e * D2D_AF + D2D_A_VY) * N;
    for (int k0 = 0; k0 < N;) {                           // every pass places at least one agent
      stream_ensure(buf, p, 4, lane);
      const int n = min(min((D2D_W_BUF - p) / 4, WAVE), N - k0);
      if (lane < n) {
        const uint32_t *g = buf + p + 4 * lane;
        double pvx, pvy;
        d2d_w_redraw(d2d_rng_temper(g[0]), d2d_rng_temper(g[1]), d2d_rng_temper(g[2]), d2d_rng_temper(g[3]), &pvx, &pvy);
        avx[k0 + lane] = pvx;
        avy[k0 + lane] = pvy;
      }
      p += 4 * n;
      k0 += n;
    }
  }

  // ---- the numpy stream: seeded key, first regeneration
  __syncthreads();
  if (lane == 0) d2d_w_init_genrand(key, seed);
  __syncthreads();
  wave_regen(key, lane);
  if (st.rng)
    for (int i = lane; i < D2D_RNG_WORDS; i += WAVE)
      st.rng[(size_t)e * D2D_RNG_WORDS + i] = !ok ? 0u : i < D2D_RNG_KEY ? key[i] : i == D2D_RNG_POS ? (uint32_t)D2D_W_NP_POS : 0u;
  if (lane == 0) s.status[e] = ok ? D2D_WORLD_OK : D2D_WORLD_CAP;
  for (int i = lane; i < 3 * P; i += WAVE) s.obstacles[(size_t)e * P * 3 + i] = ok ? pil[i] : 0;

  // ---- grids before the agents: border, pillar discs; the drone's map is unexplored
  const int G = d2d_w_grid_bytes(W, H, tile);
  uint8_t *gt = st.gt + (size_t)e * G;
  fill_bytes(gt, G, lane, [&](int f) -> uint8_t {
    int i, j;
    return (ok && d2d_w_cell_of(f, W, H, tile, &i, &j)) ? d2d_w_static_cell(i, j, W, H, scale, P, pil) : (uint8_t)0;
  });
  fill_bytes(st.dmap + (size_t)e * G, G, lane, [](int) -> uint8_t { return 0; });
  __syncthreads();   // (drains the wave's stores: the DYNAMIC cells below land behind them)

  // ---- agent records, lane = agent; then each agent's disc, wave = block of cells
  double *ag = st.agents + (size_t)e * D2D_AF * N;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    double x = 0.0, y = 0.0, r2 = 0.0;
    int ci = 0, cj = 0, u0 = 0;
    if (k < N) {
      double vx, vy, r, tr;
      if (k < nr) {
        x = acc[4 * k]; y = acc[4 * k + 1]; r = acc[4 * k + 2]; r2 = d2d_pow2(r);
        vx = -par[D2D_WE_SPEED] * s.unit[2 * k];
        vy = -par[D2D_WE_SPEED] * s.unit[2 * k + 1];
        tr = r;
      } else {
        const int32_t *c = s.cells + 3 * (size_t)(k - nr);
        x = (double)(5 + c[0] * 10); y = (double)(5 + c[1] * 10); r = 5.0; r2 = 25.0;
        vx = d2d_w_static_vel(key, c[2], par[D2D_WE_SPEED], 0);
        vy = d2d_w_static_vel(key, c[2], par[D2D_WE_SPEED], 1);
        tr = par[D2D_WE_TRK_R];
      }
      const int unit = (int)d2d_w_floordiv(r, scale);
      ci = (int)d2d_w_floordiv(x, scale);
      cj = (int)d2d_w_floordiv(y, scale);
      u0 = unit + 2;
      ag[D2D_A_PX * N + k] = ok ? x : 0.0;
      ag[D2D_A_PY * N + k] = ok ? y : 0.0;
      if (!redraw) {                                      // (a redrawn env is ok, and its lane k wrote both above)
        ag[D2D_A_VX * N + k] = ok ? vx : 0.0;
        ag[D2D_A_VY * N + k] = ok ? vy : 0.0;
      }
      ag[D2D_A_R * N + k] = ok ? r : 0.0;
      ag[D2D_A_R2 * N + k] = ok ? r2 : 0.0;
      st.agent_unit[(size_t)e * N + k] = ok ? unit : 0;
      int32_t *dp = st.dyn_prev + ((size_t)e * N + k) * 3;
      dp[0] = ok ? ci : 0;
      dp[1] = ok ? cj : 0;
      dp[2] = ok ? u0 : 0;
      s.tracker_radius[(size_t)e * N + k] = ok ? tr : 0.0;
      st.active[(size_t)e * N + k] = 0;
      if (st.kf_len) st.kf_len[(size_t)e * N + k] = ok ? 1 : 0;
    }
    const int cnt = min(WAVE, N - k0);
    for (int a = 0; ok && a < cnt; ++a) {
      const double ax = shfl_f64(x, a), ay = shfl_f64(y, a), ar2 = shfl_f64(r2, a);
      const int ai = __shfl(ci, a, WAVE), aj = __shfl(cj, a, WAVE), au = __shfl(u0, a, WAVE);
      const int side = 2 * au + 1;
      for (int c = lane; c < side * side; c += WAVE) {
        const int i = ai - au + c / side, j = aj - au + c % side;
        if (i >= 0 && i < W && j >= 0 && j < H && d2d_w_in_agent(i, j, scale, ax, ay, ar2))
          gt[d2d_w_cell_index(i, j, H, tile)] = D2D_DYNAMIC;
      }
    }
  }
  if (st.kf)
    for (int i = lane; i < N * D2D_KF; i += WAVE) st.kf[(size_t)e * N * D2D_KF + i] = ok ? d2d_w_kf_default(i % D2D_KF) : 0.0;

  // ---- drone, targets, counters
  if (lane < D2D_DF) {
    double v = 0.0;
    if (ok) v = lane == D2D_D_X ? par[D2D_WE_X0] : lane == D2D_D_Y ? par[D2D_WE_Y0] : lane == D2D_D_YAW ? 270.0 : 0.0;   // (-90) % 360
    st.drone[(size_t)e * D2D_DF + lane] = v;
  }
  if (lane < 2) st.target[(size_t)e * 2 + lane] = ok ? par[D2D_WE_X0 + lane] : 0.0;
  for (int i = lane; i < 2 * T; i += WAVE) st.targets[(size_t)e * T * 2 + i] = ok ? tgt[i] : 0.0;
  if (lane < D2D_CF) {
    int v = 0;
    if (ok) v = lane == D2D_C_SM ? D2D_SM_WAIT_FOR_GOAL : lane == D2D_C_NTGT ? (int)par[D2D_WE_NTGT] : 0;
    st.counters[(size_t)e * D2D_CF + lane] = v;
  }
