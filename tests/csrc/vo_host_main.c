/* Stand-alone sanitizer target of tests/test_vo_host_build.py: the host loops of csrc/metrics/d2d_vo.h (through vo_host.c) on
 * exactly sized heap arrays.  argv[1] is a case file the test writes -- int32 N, P, C, then doubles agents [6][N], pos [P][2],
 * cand [C][2], then int32 count [P] as the Python model expects it -- and the program runs it whole (counts compared) and cut down
 * to C = 1, C = 65, P = 1 and N = 1.  Built with -fsanitize=address,undefined; exits 0 and writes nothing to stderr. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void vo_host_geometry(const double *, const double *, double, int32_t, int32_t, int32_t, double *, double *, uint8_t *);
void vo_host_cones(const double *, const double *, const uint8_t *, int32_t, int32_t, int32_t, double *);
void vo_host_count(const double *, const double *, const double *, const uint8_t *, int32_t, int32_t, int32_t, int32_t, int32_t *);

static void *need(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

/* one world; returns the counts (the caller frees them) */
static int32_t *run(const double *agents, const double *pos, const double *cand, int N, int P, int C) {
  const size_t n = (size_t)P * N;
  double *arg = need(n * sizeof(double)), *tba = need(n * sizeof(double)), *half = need(n * sizeof(double));
  double *cone = need(2 * n * sizeof(double));
  uint8_t *col = need((size_t)P);
  int32_t *count = need((size_t)P * sizeof(int32_t));
  vo_host_geometry(agents, pos, 5.0, 1, N, P, arg, tba, col);
  for (size_t i = 0; i < n; ++i) half[i] = arg[i] > 1.0 ? 0.0 : asin(arg[i]);
  vo_host_cones(tba, half, col, 1, N, P, cone);
  vo_host_count(agents, cand, cone, col, 1, N, P, C, count);
  for (int p = 0; p < P; ++p)
    if (count[p] < -1 || count[p] > C || (count[p] == -1) != (col[p] != 0)) exit(3);
  free(arg); free(tba); free(half); free(cone); free(col);
  return count;
}

int main(int argc, char **argv) {
  if (argc < 2) return 64;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 65;
  int32_t hdr[3];
  if (fread(hdr, sizeof(int32_t), 3, f) != 3) return 66;
  const int N = hdr[0], P = hdr[1], C = hdr[2];
  if (N < 1 || P < 1 || C < 65) return 66;
  double *ag = need(sizeof(double) * 6 * N), *pos = need(sizeof(double) * 2 * P), *cand = need(sizeof(double) * 2 * C);
  int32_t *want = need(sizeof(int32_t) * P);
  if (fread(ag, sizeof(double), 6 * (size_t)N, f) != 6 * (size_t)N || fread(pos, sizeof(double), 2 * (size_t)P, f) != 2 * (size_t)P ||
      fread(cand, sizeof(double), 2 * (size_t)C, f) != 2 * (size_t)C || fread(want, sizeof(int32_t), (size_t)P, f) != (size_t)P)
    return 66;
  fclose(f);

  int32_t *got = run(ag, pos, cand, N, P, C);
  if (memcmp(got, want, sizeof(int32_t) * P)) return 4;
  free(got);
  const int cs[2] = {1, 65};
  for (int k = 0; k < 2; ++k) {   /* the first cs[k] candidates, in an array of exactly that size */
    double *c2 = need(sizeof(double) * 2 * cs[k]);
    memcpy(c2, cand, sizeof(double) * 2 * cs[k]);
    free(run(ag, pos, c2, N, P, cs[k]));
    free(c2);
  }
  for (int p = 0; p < P; ++p) {   /* every position alone: P = 1 */
    double *p1 = need(sizeof(double) * 2);
    memcpy(p1, pos + 2 * p, sizeof(double) * 2);
    got = run(ag, p1, cand, N, 1, C);
    if (got[0] != want[p]) return 5;
    free(got);
    free(p1);
  }
  double *a1 = need(sizeof(double) * 6);   /* the first agent alone: N = 1 */
  for (int r = 0; r < 6; ++r) a1[r] = ag[(size_t)r * N];
  free(run(a1, pos, cand, 1, P, C));
  free(run(a1, pos, cand, 1, 1, 1));
  free(a1);
  free(ag); free(pos); free(cand); free(want);
  return 0;
}
