/* Stand-alone sanitizer target of tests/test_jerk_host_build.py: the host loop of csrc/jerk/d2d_jerk.h (through jerk_host.c) on
 * exactly sized heap arrays.  argv[1] is a case file the test writes: int32 count, then per batch int32 B, N, S, W, H, tile, grid
 * bytes per env; doubles scale, W_px, H_px, drone_radius, agent_radius, var_cam, half_v_max; the inputs drone [B][8], target [B][2],
 * active [B][N], kf [B][N][20], dmap [B][bytes], trk_radius [B][N], trk_prev [B][N], th_tab [72][8], tt_tab [72][S][5], tie_perm and
 * tie_eq [288][72]; and what the Python model expects: plan_ok [B], wp [B][6], int32 choice [B], trk_radius [B][N].  Built with
 * -fsanitize=address,undefined; exits 0 and writes nothing to stderr. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/d2d_jerk.h"

int jerk_host_plan(const d2d_jerk_call *, double *);
void jerk_host_reset(double *, uint8_t *, const double *, const uint8_t *, int32_t, int32_t, int32_t);

static void *need(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

static void *take(FILE *f, size_t n) {
  void *p = need(n);
  if (n && fread(p, 1, n, f) != n) exit(66);
  return p;
}

int main(int argc, char **argv) {
  if (argc < 2) return 64;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 65;
  int32_t *count = take(f, sizeof(int32_t));
  for (int s = 0; s < *count; ++s) {
    int32_t *h = take(f, sizeof(int32_t) * 7);
    double *d = take(f, sizeof(double) * 7);
    const size_t B = (size_t)h[0], N = (size_t)h[1], S = (size_t)h[2], gb = (size_t)h[6];
    if (h[0] < 1 || h[1] < 0 || h[2] < 1) return 66;
    d2d_jerk_call c;
    memset(&c, 0, sizeof c);
    c.B = h[0]; c.N = h[1]; c.S = h[2]; c.W = h[3]; c.H = h[4]; c.grid_tile = h[5];
    c.scale = d[0]; c.W_px = d[1]; c.H_px = d[2]; c.drone_radius = d[3]; c.agent_radius = d[4]; c.var_cam = d[5]; c.half_v_max = d[6];
    double *drone = take(f, 8 * B * 8), *target = take(f, 8 * B * 2);
    uint8_t *active = take(f, B * N);
    double *kf = take(f, 8 * B * N * 20);
    uint8_t *dmap = take(f, B * gb);
    double *radius = take(f, 8 * B * N);
    uint8_t *prev = take(f, B * N);
    double *th = take(f, 8 * 72 * 8), *tt = take(f, 8 * 72 * S * 5);
    uint8_t *perm = take(f, 288 * 72), *eq = take(f, 288 * 72);
    uint8_t *want_ok = take(f, B);
    double *want_wp = take(f, 8 * B * 6);
    int32_t *want_choice = take(f, 4 * B);
    double *want_radius = take(f, 8 * B * N);
    uint8_t *ok = need(B), *valid = need(B);
    double *wp = need(8 * B * 6), *work = need(8 * 5 * (N ? N : 1)), *radius0 = need(8 * B * N);
    int32_t *choice = need(4 * B), *stat = need(4 * B);
    memcpy(radius0, radius, 8 * B * N);
    c.drone = drone; c.target = target; c.active = active; c.kf = kf; c.dmap = dmap; c.trk_radius = radius; c.trk_prev = prev;
    c.th_tab = th; c.tt_tab = tt; c.tie_perm = perm; c.tie_eq = eq;
    c.plan_ok = ok; c.wp_valid = valid; c.wp = wp; c.choice = choice; c.stat = stat;
    if (jerk_host_plan(&c, work)) return 3;
    if (memcmp(ok, want_ok, B) || memcmp(valid, want_ok, B)) return 4;
    if (memcmp(wp, want_wp, 8 * B * 6)) return 5;
    if (memcmp(choice, want_choice, 4 * B)) return 6;
    if (memcmp(radius, want_radius, 8 * B * N)) return 7;
    jerk_host_reset(radius, prev, radius0, NULL, 1, c.B, c.N);
    if (memcmp(radius, radius0, 8 * B * N)) return 8;
    for (size_t i = 0; i < B * N; ++i)
      if (prev[i]) return 9;
    free(h); free(d); free(drone); free(target); free(active); free(kf); free(dmap); free(radius); free(prev); free(th); free(tt);
    free(perm); free(eq); free(want_ok); free(want_wp); free(want_choice); free(want_radius); free(ok); free(valid); free(wp);
    free(work); free(radius0); free(choice); free(stat);
  }
  fclose(f);
  free(count);
  return 0;
}
