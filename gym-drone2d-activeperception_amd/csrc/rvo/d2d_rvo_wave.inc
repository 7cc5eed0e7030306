  // d2d_rvo_wave.inc -- the body of one rvo_velocity wave (d2d_rvo.hip), included as text by rvo_velocity_kernel and, behind its test of
  // the env's done flag, by rvo_velocity_live_kernel.  Text and not an inlined function: rvo_velocity_kernel then compiles to the very
  // instructions it had while the body stood in it.  Names of the including kernel: agents, vel, pillars, N, P, vel_out.
  extern __shared__ __attribute__((aligned(16))) double cones[];   // [6][nc]
  const int lane = threadIdx.x;
  const int i = (int)(blockIdx.x % (unsigned)N);
  const size_t b = blockIdx.x / (unsigned)N;
  const int nc = N - 1 + P;
  const double *ag = agents + b * D2D_AF * N, *v = vel + b * 2 * N;
  const int32_t *pil = pillars + b * P * 3;                          // (not read when P == 0)
  const double rob_rad = ag[D2D_A_R * N] + 0.01;
  const double pax = ag[D2D_A_PX * N + i], pay = ag[D2D_A_PY * N + i];
  const double prefx = ag[D2D_A_VX * N + i], prefy = ag[D2D_A_VY * N + i];

  for (int k = lane; k < nc; k += WAVE) d2d_rvo_cone_of(ag, v, pil, N, i, k, rob_rad, cones + k, (size_t)nc);
  __syncthreads();
  const double *apx = cones, *apy = cones + nc, *right = cones + 2 * nc, *left = cones + 3 * nc, *dist = cones + 4 * nc,
               *rad = cones + 5 * nc;

  double delta;
  const int nrad = d2d_rvo_radii(d2d_vo_norm(prefx, prefy), &delta);
  const int C = D2D_RVO_NTHETA * nrad + 1;

  double best_key = INFINITY;
  int best = NO_INDEX;
  for (int c0 = 0; c0 < C; c0 += WAVE) {            // min(suitable_V, key=norm(v - pref))
    const int c = c0 + lane;
    double cx, cy, td, dx, dy;
    d2d_rvo_candidate(c < C ? c : C - 1, nrad, delta, prefx, prefy, &cx, &cy);
    bool suit = c < C;
    for (int k = 0; k < nc; ++k) {
      if (__ballot(suit) == 0ull) break;
      if (suit && d2d_rvo_inside(cx, cy, pax, pay, apx[k], apy[k], right[k], left[k], &td, &dx, &dy)) suit = false;
    }
    if (suit) {
      const double key = d2d_vo_norm(cx - prefx, cy - prefy);
      if (key < best_key) best_key = key, best = c;  // (never a NaN, never +inf: the first candidate of the lane always enters)
    }
  }
  if (__ballot(best != NO_INDEX) == 0ull) {          // min(unsuitable_V, key=0.2 / tc_V + norm(v - pref)): every candidate
    for (int c0 = 0; c0 < C; c0 += WAVE) {
      const int c = c0 + lane;
      if (c >= C) continue;
      double cx, cy, td, dx, dy, tc = 0.0;
      bool have = false;
      d2d_rvo_candidate(c, nrad, delta, prefx, prefy, &cx, &cy);
      for (int k = 0; k < nc; ++k)
        if (d2d_rvo_inside(cx, cy, pax, pay, apx[k], apy[k], right[k], left[k], &td, &dx, &dy)) {
          const double t = d2d_rvo_tc(td, dx, dy, right[k], left[k], dist[k], rad[k]);
          if (!have || t < tc) tc = t;
          have = true;
        }
      double key = d2d_rvo_key(tc, cx, cy, prefx, prefy);
      if (key != key) {
        if (c != 0) continue;                        // a NaN that is not the list's first element never wins
        key = -INFINITY;                             // the first element does, whatever follows (every other key is >= 0)
      }
      if (key < best_key || (key == best_key && c < best)) best_key = key, best = c;
    }
  }
#pragma unroll
  for (int m = WAVE / 2; m > 0; m >>= 1) {
    const double ok = __shfl_xor(best_key, m, WAVE);
    const int oi = __shfl_xor(best, m, WAVE);
    if (ok < best_key || (ok == best_key && oi < best)) best_key = ok, best = oi;
  }
  if (lane == 0) {
    double cx, cy;
    d2d_rvo_candidate(best, nrad, delta, prefx, prefy, &cx, &cy);
    double *out = vel_out + b * 2 * N;
    out[i] = cx;
    out[N + i] = cy;
  }
