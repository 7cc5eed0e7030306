/*
 * d2d_worlds.h — restatement of the reference's world construction (include/d2d_worlds.h names the reference lines).
 *
 * Two random streams, both MT19937 (Matsumoto & Nishimura), both seeded with map_id:
 *
 *   Python's `random`   random.seed(int) is init_genrand(19650218) followed by init_by_array with the one-word key [map_id]
 *                       (CPython Modules/_randommodule.c): two serial passes of 624 and 623 steps, then mt[0] = 0x80000000,
 *                       position 624.  random() is the 53-bit double of two tempered words (>> 5, >> 6), uniform(a, b) is
 *                       a + (b - a) * random(), randint(a, b) is a + _randbelow(b - a + 1) with k = n.bit_length(),
 *                       r = word >> (32 - k), redrawn while r >= n (Lib/random.py).  Places the pillars and the agents.
 *   numpy's global      RandomState(int) is init_genrand(map_id) (numpy/random/_mt19937.pyx, _legacy_seeding).  The 100 rand()
 *                       of the static map's velocities take words 0 .. 199 of the first regenerated key; that key with
 *                       position 200 is what the env keeps (d2d_state.rng).
 *
 * The scalar pieces below are shared by the device kernel (d2d_worlds.hip) and by the plain sequential form at the end of this
 * file (host builds only), which the CPU tests compare with host_init.init_world field by field.
 *
 * Must be compiled with -ffp-contract=off: the reference performs no fused multiply-add in any of this.
 */
#ifndef D2D_WORLDS_IMPL_H
#define D2D_WORLDS_IMPL_H

#include <math.h>
#include <stdint.h>

#include "../../../include/d2d_worlds.h"

#ifndef D2D_WORLDS_QUAL
#define D2D_WORLDS_QUAL static inline
#endif
#ifndef D2D_RNG_QUAL
#define D2D_RNG_QUAL D2D_WORLDS_QUAL
#endif
#ifndef D2D_SINCOS_QUAL
#define D2D_SINCOS_QUAL D2D_WORLDS_QUAL
#endif
#ifndef D2D_POW2_QUAL
#define D2D_POW2_QUAL D2D_WORLDS_QUAL
#endif
#include "../d2d_pow2.h"
#include "../d2d_rng.h"
#include "../d2d_sincos.h"

#define D2D_W_CARRY 8                            /* words in front of the key that hold what a regeneration left undrawn */
#define D2D_W_BUF (D2D_W_CARRY + D2D_RNG_KEY)    /* words of the Python stream's buffer */
#define D2D_W_ACC_F 4                            /* doubles per accepted agent: x, y, r, pow(r, 2.0) */
#define D2D_W_NP_POS 200                         /* numpy's position after the 100 rand() of drone_v2.py:50-53 */

/* init_genrand's recurrence: word i from word i - 1 */
D2D_WORLDS_QUAL uint32_t d2d_w_genrand_next(uint32_t prev, uint32_t i) { return 1812433253u * (prev ^ (prev >> 30)) + i; }

/* init_genrand(seed) into mt[624] */
D2D_WORLDS_QUAL void d2d_w_init_genrand(uint32_t *mt, uint32_t seed) {
  mt[0] = seed;
  for (uint32_t i = 1; i < D2D_RNG_KEY; ++i) mt[i] = d2d_w_genrand_next(mt[i - 1], i);
}

/* random.seed(seed), 0 <= seed < 2**32, into mt[624]; the position is 624 */
D2D_WORLDS_QUAL void d2d_w_seed_python(uint32_t *mt, uint32_t seed) {
  d2d_w_init_genrand(mt, 19650218u);
  uint32_t i = 1;
  for (int k = 0; k < D2D_RNG_KEY; ++k) { /* init_by_array, key = [seed]: j stays 0 */
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + seed;
    if (++i >= D2D_RNG_KEY) {
      mt[0] = mt[D2D_RNG_KEY - 1];
      i = 1;
    }
  }
  for (int k = 0; k < D2D_RNG_KEY - 1; ++k) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - i;
    if (++i >= D2D_RNG_KEY) {
      mt[0] = mt[D2D_RNG_KEY - 1];
      i = 1;
    }
  }
  mt[0] = 0x80000000u;
}

/* n.bit_length(), n > 0 */
D2D_WORLDS_QUAL int d2d_w_bit_length(uint32_t n) {
  int k = 0;
  for (int b = 0; b < 32; ++b)
    if (n >> b) k = b + 1;
  return k;
}

/* a + (b - a) * random() from the two tempered words of random(); w = b - a */
D2D_WORLDS_QUAL double d2d_w_uniform(double a, double w, uint32_t g0, uint32_t g1) { return a + w * d2d_rng_double(g0, g1); }

/* validation_speed.py:136-138 for one agent: the preferred velocity from the four tempered words of two random().  The
 * arithmetic is the script's, operand for operand: random() * 40 + 20, random() * 2 * np.pi, vel * np.cos / np.sin(angle) */
D2D_WORLDS_QUAL void d2d_w_redraw(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3, double *pvx, double *pvy) {
  const double vel = d2d_rng_double(g0, g1) * 40.0 + 20.0;
  const double angle = (d2d_rng_double(g2, g3) * 2.0) * 3.141592653589793;
  *pvx = vel * d2d_cos(angle);
  *pvy = vel * d2d_sin(angle);
}

/* numpy.linalg.norm of a 2-vector: sqrt(x . x) */
D2D_WORLDS_QUAL double d2d_w_norm(double dx, double dy) { return sqrt(dx * dx + dy * dy); }

/* Python's and numpy's float `a // b` for b > 0 (Objects/floatobject.c float_floor_div; npy_divmod is the same algorithm) */
D2D_WORLDS_QUAL double d2d_w_floordiv(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && mod < 0.0) div -= 1.0;
  if (div == 0.0) return copysign(0.0, a / b);
  double fl = floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl;
}

/* byte of cell (i, j) inside one env's grid: row-major [W][H], or 16 x 16 tiles row-major over (ceil(W / 16), ceil(H / 16)) */
D2D_WORLDS_QUAL int d2d_w_grid_bytes(int W, int H, int tile) {
  return tile ? ((W + tile - 1) / tile) * ((H + tile - 1) / tile) * tile * tile : W * H;
}
D2D_WORLDS_QUAL int d2d_w_cell_index(int i, int j, int H, int tile) {
  if (!tile) return i * H + j;
  const int Ht = (H + tile - 1) / tile;
  return ((i / tile) * Ht + j / tile) * tile * tile + (i % tile) * tile + j % tile;
}
/* the inverse: cell (i, j) of byte `flat`; returns 0 for a byte of the tile padding */
D2D_WORLDS_QUAL int d2d_w_cell_of(int flat, int W, int H, int tile, int *i, int *j) {
  if (!tile) {
    *i = flat / H;
    *j = flat - *i * H;
    return 1;
  }
  const int Ht = (H + tile - 1) / tile, t = flat / (tile * tile), c = flat - t * tile * tile;
  *i = (t / Ht) * tile + c / tile;
  *j = (t % Ht) * tile + c % tile;
  return *i < W && *j < H;
}

/* utils.py:495-520 for one cell before the agents: the border and the pillar discs are OCCUPIED.  pillars: [P][3] */
D2D_WORLDS_QUAL uint8_t d2d_w_static_cell(int i, int j, int W, int H, double scale, int P, const int32_t *pillars) {
  if (i == 0 || j == 0 || i == W - 1 || j == H - 1) return D2D_OCCUPIED;
  const double cx = scale * ((double)i + 0.5), cy = scale * ((double)j + 0.5); /* get_real_pos, utils.py:542 */
  for (int q = 0; q < P; ++q) {
    const double dx = cx - (double)pillars[3 * q], dy = cy - (double)pillars[3 * q + 1];
    if (sqrt(dx * dx + dy * dy) <= (double)pillars[3 * q + 2]) return D2D_OCCUPIED;
  }
  return D2D_UNOCCUPIED;
}

/* utils.py:521-525: is the centre of cell (i, j) inside the agent's disc */
D2D_WORLDS_QUAL int d2d_w_in_agent(int i, int j, double scale, double ax, double ay, double r2) {
  const double dx = scale * ((double)i + 0.5) - ax, dy = scale * ((double)j + 0.5) - ay;
  return dx * dx + dy * dy <= r2;
}

/* does a pillar candidate (integers) keep clear of the targets and the start, drone_v2.py:17-24.  par: the env's env_par row */
D2D_WORLDS_QUAL int d2d_w_pillar_free(int ox, int oy, int orad, const double *par, const double *tgt, double pillar_clear,
                                      double start_clear) {
  int free_ = 1;
  const int nt = (int)par[D2D_WE_NTGT];
  for (int t = 0; t < nt; ++t)
    if (d2d_w_norm(tgt[2 * t] - (double)ox, tgt[2 * t + 1] - (double)oy) <= pillar_clear + (double)orad) free_ = 0;
  if (d2d_w_norm(par[D2D_WE_X0] - (double)ox, par[D2D_WE_Y0] - (double)oy) <= start_clear) free_ = 0;
  return free_;
}

/* does an agent candidate keep clear of the pillars and the start, drone_v2.py:40-44 */
D2D_WORLDS_QUAL int d2d_w_agent_free_static(double x, double y, double r, const double *par, int P, const int32_t *pillars,
                                            double start_clear) {
  int free_ = 1;
  for (int q = 0; q < P; ++q)
    if (d2d_w_norm((double)pillars[3 * q] - x, (double)pillars[3 * q + 1] - y) <= (double)pillars[3 * q + 2] + r + 10.0) free_ = 0;
  if (d2d_w_norm(x - par[D2D_WE_X0], y - par[D2D_WE_Y0]) <= start_clear) free_ = 0;
  return free_;
}

/* velocity component of the static-map agents with label `label`, drone_v2.py:50-53: speed * cos / sin(rand() * 2 * pi) of draw
 * `label` of the numpy stream; key: the first regenerated key */
D2D_WORLDS_QUAL double d2d_w_static_vel(const uint32_t *key, int label, double speed, int is_sin) {
  const double d = d2d_rng_double(d2d_rng_temper(key[2 * label]), d2d_rng_temper(key[2 * label + 1]));
  const double direction = d * 2.0 * 3.141592653589793;
  return speed * (is_sin ? d2d_sin(direction) : d2d_cos(direction));
}

/* value k of an env's kf record at rest: Sigma = diag(1, 1, 10, 10) behind mu[4], utils.py:181 */
D2D_WORLDS_QUAL double d2d_w_kf_default(int k) { return (k == 4 || k == 9) ? 1.0 : (k == 14 || k == 19) ? 10.0 : 0.0; }

#if !defined(__HIPCC__)
/* The whole construction of env e, one attempt after the other, on HOST pointers.  `buf`: D2D_W_BUF words, `acc`:
 * n_rand * D2D_W_ACC_F doubles of scratch. */
D2D_WORLDS_QUAL void d2d_worlds_build_seq_env(const d2d_world_spec *s, const d2d_state *st, int e, uint32_t *buf, double *acc) {
  const int N = s->N, nr = s->n_rand, P = s->P, T = s->T, W = s->W, H = s->H, tile = s->grid_tile;
  const int G = d2d_w_grid_bytes(W, H, tile);
  const double *par = s->env_par + (size_t)e * D2D_WORLDS_ENV_F, *tgt = s->env_tgt + (size_t)e * T * 2;
  const double scale = (double)s->scale;
  int32_t *pil = s->obstacles + (size_t)e * P * 3;
  uint32_t *key = buf + D2D_W_CARRY;
  int pos = D2D_RNG_KEY, attempts = 0, ok = 1;
  d2d_w_seed_python(key, s->map_id[e]);
#define D2D_W_NEXT(dst)                                                                                            \
  do {                                                                                                             \
    if (pos >= D2D_RNG_KEY) {                                                                                      \
      for (int i_ = 0; i_ < D2D_RNG_KEY; ++i_)                                                                     \
        key[i_] = d2d_rng_twist(key[i_], key[(i_ + 1) % D2D_RNG_KEY], key[(i_ + D2D_RNG_M) % D2D_RNG_KEY]);        \
      pos = 0;                                                                                                     \
    }                                                                                                              \
    (dst) = d2d_rng_temper(key[pos++]);                                                                            \
  } while (0)
  /* pillars */
  const uint32_t pn[3] = {(uint32_t)(s->W_px - 99), (uint32_t)(s->H_px - 99), 6u};
  const int plo[3] = {50, 50, 15};
  int np_ = 0;
  while (ok && np_ < P) {
    if (attempts >= s->max_attempts) { ok = 0; break; }
    attempts += 1;
    int v[3];
    for (int c = 0; c < 3 && ok; ++c) {
      const int k = d2d_w_bit_length(pn[c]);
      for (;;) {
        uint32_t g;
        D2D_W_NEXT(g);
        const uint32_t r = g >> (32 - k);
        if (r < pn[c]) { v[c] = plo[c] + (int)r; break; }
        if (++attempts >= s->max_attempts) { ok = 0; break; }
      }
    }
    if (!ok) break;
    if (d2d_w_pillar_free(v[0], v[1], v[2], par, tgt, s->pillar_clear, s->start_clear)) {
      pil[3 * np_] = v[0]; pil[3 * np_ + 1] = v[1]; pil[3 * np_ + 2] = v[2];
      np_ += 1;
    }
  }
  /* agents */
  int na = 0;
  while (ok && na < nr) {
    if (attempts >= s->max_attempts) { ok = 0; break; }
    attempts += 1;
    uint32_t g[6];
    for (int c = 0; c < 6; ++c) D2D_W_NEXT(g[c]);
    const double x = d2d_w_uniform(20.0, (double)(s->W_px - 20 - 20), g[0], g[1]);
    const double y = d2d_w_uniform(20.0, (double)(s->H_px - 20 - 20), g[2], g[3]);
    const double r = d2d_w_uniform(par[D2D_WE_R_LO], par[D2D_WE_R_W], g[4], g[5]);
    int free_ = d2d_w_agent_free_static(x, y, r, par, P, pil, s->start_clear);
    for (int q = 0; q < na; ++q)
      if (d2d_w_norm(acc[4 * q] - x, acc[4 * q + 1] - y) <= acc[4 * q + 2] + r) free_ = 0;
    if (free_) {
      acc[4 * na] = x; acc[4 * na + 1] = y; acc[4 * na + 2] = r; acc[4 * na + 3] = d2d_pow2(r);
      na += 1;
    }
  }
  /* the redraw (D2D_WE_REDRAW): the stream goes on where the last agent left it, before its key makes room for numpy's */
  const int redraw = ok && par[D2D_WE_REDRAW] != 0.0;
  double *ag = st->agents + (size_t)e * D2D_AF * N;
  for (int k = 0; redraw && k < N; ++k) {
    uint32_t g[4];
    for (int c = 0; c < 4; ++c) D2D_W_NEXT(g[c]);
    d2d_w_redraw(g[0], g[1], g[2], g[3], &ag[D2D_A_VX * N + k], &ag[D2D_A_VY * N + k]);
  }
#undef D2D_W_NEXT
  /* the numpy stream: seeded key, first regeneration */
  d2d_w_init_genrand(key, s->map_id[e]);
  for (int i = 0; i < D2D_RNG_KEY; ++i)
    key[i] = d2d_rng_twist(key[i], key[(i + 1) % D2D_RNG_KEY], key[(i + D2D_RNG_M) % D2D_RNG_KEY]);
  if (st->rng)
    for (int i = 0; i < D2D_RNG_WORDS; ++i)
      st->rng[(size_t)e * D2D_RNG_WORDS + i] = !ok ? 0u : i < D2D_RNG_KEY ? key[i] : i == D2D_RNG_POS ? (uint32_t)D2D_W_NP_POS : 0u;
  s->status[e] = ok ? D2D_WORLD_OK : D2D_WORLD_CAP;
  if (!ok)
    for (int i = 0; i < 3 * P; ++i) pil[i] = 0;
  /* agent records */
  for (int k = 0; k < N; ++k) {
    double x, y, vx, vy, r, r2, tr;
    if (k < nr) {
      x = acc[4 * k]; y = acc[4 * k + 1]; r = acc[4 * k + 2]; r2 = acc[4 * k + 3];
      vx = -par[D2D_WE_SPEED] * s->unit[2 * k];
      vy = -par[D2D_WE_SPEED] * s->unit[2 * k + 1];
      tr = r;
    } else {
      const int32_t *c = s->cells + 3 * (k - nr);
      x = (double)(5 + c[0] * 10); y = (double)(5 + c[1] * 10); r = 5.0; r2 = 25.0;
      vx = d2d_w_static_vel(key, c[2], par[D2D_WE_SPEED], 0);
      vy = d2d_w_static_vel(key, c[2], par[D2D_WE_SPEED], 1);
      tr = par[D2D_WE_TRK_R];
    }
    const int unit = (int)d2d_w_floordiv(r, scale);
    const double rec[D2D_AF] = {x, y, vx, vy, r, r2};
    for (int f = 0; f < D2D_AF; ++f)
      if (!(redraw && (f == D2D_A_VX || f == D2D_A_VY))) ag[f * N + k] = ok ? rec[f] : 0.0;
    st->agent_unit[(size_t)e * N + k] = ok ? unit : 0;
    int32_t *dp = st->dyn_prev + ((size_t)e * N + k) * 3;
    dp[0] = ok ? (int)d2d_w_floordiv(x, scale) : 0;
    dp[1] = ok ? (int)d2d_w_floordiv(y, scale) : 0;
    dp[2] = ok ? unit + 2 : 0;
    s->tracker_radius[(size_t)e * N + k] = ok ? tr : 0.0;
    st->active[(size_t)e * N + k] = 0;
    if (st->kf)
      for (int f = 0; f < D2D_KF; ++f) st->kf[((size_t)e * N + k) * D2D_KF + f] = ok ? d2d_w_kf_default(f) : 0.0;
    if (st->kf_len) st->kf_len[(size_t)e * N + k] = ok ? 1 : 0;
  }
  /* grids */
  uint8_t *gt = st->gt + (size_t)e * G, *dm = st->dmap + (size_t)e * G;
  for (int f = 0; f < G; ++f) {
    int i, j;
    gt[f] = (ok && d2d_w_cell_of(f, W, H, tile, &i, &j)) ? d2d_w_static_cell(i, j, W, H, scale, P, pil) : 0;
    dm[f] = 0;
  }
  for (int k = 0; ok && k < N; ++k) {
    const double ax = ag[D2D_A_PX * N + k], ay = ag[D2D_A_PY * N + k], r2 = ag[D2D_A_R2 * N + k];
    const int32_t *dp = st->dyn_prev + ((size_t)e * N + k) * 3;
    for (int i = dp[0] - dp[2]; i <= dp[0] + dp[2]; ++i)
      for (int j = dp[1] - dp[2]; j <= dp[1] + dp[2]; ++j)
        if (i >= 0 && i < W && j >= 0 && j < H && d2d_w_in_agent(i, j, scale, ax, ay, r2))
          gt[d2d_w_cell_index(i, j, H, tile)] = D2D_DYNAMIC;
  }
  /* drone, targets, counters */
  double *dr = st->drone + (size_t)e * D2D_DF;
  for (int f = 0; f < D2D_DF; ++f) dr[f] = 0.0;
  if (ok) { dr[D2D_D_X] = par[D2D_WE_X0]; dr[D2D_D_Y] = par[D2D_WE_Y0]; dr[D2D_D_YAW] = 270.0; } /* (-90) % 360, utils.py:718 */
  st->target[(size_t)e * 2] = ok ? par[D2D_WE_X0] : 0.0;
  st->target[(size_t)e * 2 + 1] = ok ? par[D2D_WE_Y0] : 0.0;
  for (int f = 0; f < 2 * T; ++f) st->targets[(size_t)e * T * 2 + f] = ok ? tgt[f] : 0.0;
  for (int f = 0; f < D2D_CF; ++f) st->counters[(size_t)e * D2D_CF + f] = 0;
  if (ok) {
    st->counters[(size_t)e * D2D_CF + D2D_C_SM] = D2D_SM_WAIT_FOR_GOAL; /* drone_v2.py:116 */
    st->counters[(size_t)e * D2D_CF + D2D_C_NTGT] = (int32_t)par[D2D_WE_NTGT];
  }
}
#endif

#endif /* D2D_WORLDS_IMPL_H */
