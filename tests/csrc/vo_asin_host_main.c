/* Stand-alone sanitizer target of tests/test_vo_device_asin_host_build.py: d2d_vo_cones_arg_seq and d2d_asin (through
 * vo_asin_host.c) on exactly sized heap arrays.  argv[1] is a case file the test writes -- int32 N, P, then doubles agents [6][N],
 * pos [P][2], then doubles half [P][N] and cone [P][N][2] as the Python model expects them.  The program runs the world whole (with
 * and without half_out, bits compared), every position alone and the first agent alone, then d2d_asin over +-`SPAN` consecutive
 * doubles around each of its cuts in both signs, over both tables' every row and over the special values, each checked against the
 * program's own libm.  Built with -fsanitize=address,undefined: an index outside either table ends it.  Exits 0 and writes
 * nothing to stderr. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void vo_host_geometry(const double *, const double *, double, int32_t, int32_t, int32_t, double *, double *, uint8_t *);
void vo_host_cones_arg(const double *, const double *, const uint8_t *, int32_t, int32_t, int32_t, double *, double *);
void vo_host_asin(const double *, int64_t, double *);

#define SPAN 3000

static void *need(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

/* one world; half and cone (the caller frees them) */
static void run(const double *agents, const double *pos, int N, int P, double **half_out, double **cone_out) {
  const size_t n = (size_t)P * N;
  double *arg = need(n * sizeof(double)), *tba = need(n * sizeof(double)), *half = need(n * sizeof(double));
  double *cone = need(2 * n * sizeof(double)), *cone2 = need(2 * n * sizeof(double));
  uint8_t *col = need((size_t)P);
  vo_host_geometry(agents, pos, 5.0, 1, N, P, arg, tba, col);
  memset(half, 0x7f, n * sizeof(double));
  memset(cone, 0x7f, 2 * n * sizeof(double));
  memset(cone2, 0x7f, 2 * n * sizeof(double));
  vo_host_cones_arg(tba, arg, col, 1, N, P, half, cone);
  vo_host_cones_arg(tba, arg, col, 1, N, P, NULL, cone2);
  if (memcmp(cone, cone2, 2 * n * sizeof(double))) exit(3);
  free(arg); free(tba); free(col); free(cone2);
  *half_out = half;
  *cone_out = cone;
}

static int same(double a, double b) { return (isnan(a) && isnan(b)) || !memcmp(&a, &b, sizeof a); }

/* d2d_asin over an exactly sized array, against libm */
static void sweep(const double *x, int64_t n) {
  double *in = need((size_t)n * sizeof(double)), *out = need((size_t)n * sizeof(double));
  memcpy(in, x, (size_t)n * sizeof(double));
  vo_host_asin(in, n, out);
  for (int64_t i = 0; i < n; ++i)
    if (!same(out[i], asin(in[i]))) exit(6);
  free(in); free(out);
}

int main(int argc, char **argv) {
  if (argc < 2) return 64;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 65;
  int32_t hdr[2];
  if (fread(hdr, sizeof(int32_t), 2, f) != 2) return 66;
  const int N = hdr[0], P = hdr[1];
  if (N < 1 || P < 1) return 66;
  const size_t n = (size_t)P * N;
  double *ag = need(sizeof(double) * 6 * N), *pos = need(sizeof(double) * 2 * P);
  double *want_half = need(sizeof(double) * n), *want_cone = need(sizeof(double) * 2 * n);
  if (fread(ag, sizeof(double), 6 * (size_t)N, f) != 6 * (size_t)N || fread(pos, sizeof(double), 2 * (size_t)P, f) != 2 * (size_t)P ||
      fread(want_half, sizeof(double), n, f) != n || fread(want_cone, sizeof(double), 2 * n, f) != 2 * n)
    return 66;
  fclose(f);

  double *half, *cone;
  run(ag, pos, N, P, &half, &cone);
  if (memcmp(half, want_half, sizeof(double) * n)) return 4;
  if (memcmp(cone, want_cone, sizeof(double) * 2 * n)) return 5;
  free(half); free(cone);
  for (int p = 0; p < P; ++p) {   /* every position alone: P = 1 */
    double *p1 = need(sizeof(double) * 2);
    memcpy(p1, pos + 2 * p, sizeof(double) * 2);
    run(ag, p1, N, 1, &half, &cone);
    if (memcmp(half, want_half + (size_t)p * N, sizeof(double) * N)) return 7;
    if (memcmp(cone, want_cone + 2 * (size_t)p * N, sizeof(double) * 2 * N)) return 8;
    free(half); free(cone); free(p1);
  }
  double *a1 = need(sizeof(double) * 6);   /* the first agent alone: N = 1 */
  for (int r = 0; r < 6; ++r) a1[r] = ag[(size_t)r * N];
  run(a1, pos, 1, P, &half, &cone);
  free(half); free(cone); free(a1);
  free(ag); free(pos); free(want_half); free(want_cone);

  /* the asin alone: the neighbourhoods of its cuts, in both signs */
  const double cuts[9] = {0x1p-26, 0.125, 0.25, 0.5, 0.75, 0.921875, 0.953125, 0.96875, 1.0};
  double *w = need(sizeof(double) * 2 * (2 * SPAN + 1));
  for (int c = 0; c < 9; ++c) {
    int64_t b;
    memcpy(&b, &cuts[c], 8);
    for (int i = 0; i <= 2 * SPAN; ++i) {
      const int64_t v = b - SPAN + i;
      memcpy(&w[2 * i], &v, 8);
      w[2 * i + 1] = -w[2 * i];
    }
    sweep(w, 2 * (2 * SPAN + 1));
  }
  free(w);
  /* every table row (256 steps of 2^-8 over [0, 1)) and every root seed (z = (1 - x) / 2 over its 25 binades), at three points each */
  double *g = need(sizeof(double) * 2 * 3 * 256);
  for (int i = 0; i < 256; ++i)
    for (int j = 0; j < 3; ++j) {
      g[2 * (3 * i + j)] = (i + (j == 0 ? 0.0 : j == 1 ? 0.5 : 0.99999999)) / 256.0;
      g[2 * (3 * i + j) + 1] = -g[2 * (3 * i + j)];
    }
  sweep(g, 2 * 3 * 256);
  free(g);
  double *z = need(sizeof(double) * 49 * 64 * 2);
  int64_t m = 0;
  for (int e = 6; e <= 54; ++e)                      /* 1 - x = 2^-(e - 1) (1 + k / 64): z of every exponent parity and seed */
    for (int k = 0; k < 64; ++k) {
      const double x = 1.0 - ldexp(1.0 + k / 64.0, -(e - 1));
      z[m++] = x;
      z[m++] = -x;
    }
  sweep(z, m);
  free(z);
  const double sp[] = {0.0, -0.0, 1.0, -1.0, 0x1.0000000000001p+0, -0x1.0000000000001p+0, INFINITY, -INFINITY, NAN, 0x1p-1074, -0x1p-1074,
                       0x1p-1022, 2.0, -2.0, 0x1.fffffffffffffp-1, -0x1.fffffffffffffp-1};
  sweep(sp, (int64_t)(sizeof sp / sizeof sp[0]));
  return 0;
}
