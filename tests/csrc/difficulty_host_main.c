/* Stand-alone sanitizer target of tests/test_difficulty_host_build.py: the host loops of csrc/metrics/d2d_difficulty.h (through
 * difficulty_host.c) on exactly sized heap arrays.  argv[1] is a case file the test writes -- int32 W, H, S, N, P, checks, then u8
 * gt [W][H], int32 starts [S][2], int32 steps [S][8], doubles agents [6][N], pos [P][2], int32 first [P], doubles agents_end [6][N]
 * as the Python model expects them -- and the program runs it whole (results compared) and cut down to S = 1, P = 1, N = 1,
 * checks = 0 and agents_out = NULL.  Built with -fsanitize=address,undefined; exits 0 and writes nothing to stderr. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void difficulty_host_trav_steps(const uint8_t *, int32_t, int32_t, int32_t, const int32_t *, int32_t, int32_t *);
void difficulty_host_fit_first_hit(const double *, const double *, double, double, double, double, double, int32_t, int32_t, int32_t,
                                   int32_t, int32_t *, double *, double *);

static void *need(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) exit(2);
  return p;
}

static void *take(FILE *f, size_t n) {
  void *p = need(n);
  if (fread(p, 1, n, f) != n) exit(66);
  return p;
}

/* one world; returns first (the caller frees it); end: 6 * N doubles or NULL */
static int32_t *fit(const double *agents, const double *pos, int N, int P, int checks, double *end) {
  int32_t *first = need(sizeof(int32_t) * P);
  double *work = need(sizeof(double) * 5 * N);
  difficulty_host_fit_first_hit(agents, pos, 10.0, 500.0, 500.0, 10.0, 0.1, 1, N, P, checks, first, end, work);
  for (int p = 0; p < P; ++p)
    if (first[p] < -1 || first[p] >= checks) exit(3);
  free(work);
  return first;
}

int main(int argc, char **argv) {
  if (argc < 2) return 64;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 65;
  int32_t *hdr = take(f, sizeof(int32_t) * 6);
  const int W = hdr[0], H = hdr[1], S = hdr[2], N = hdr[3], P = hdr[4], checks = hdr[5];
  if (W < 1 || H < 1 || S < 1 || N < 1 || P < 1 || checks < 1) return 66;
  uint8_t *gt = take(f, (size_t)W * H);
  int32_t *starts = take(f, sizeof(int32_t) * 2 * S), *want_steps = take(f, sizeof(int32_t) * 8 * S);
  double *ag = take(f, sizeof(double) * 6 * N), *pos = take(f, sizeof(double) * 2 * P);
  int32_t *want_first = take(f, sizeof(int32_t) * P);
  double *want_end = take(f, sizeof(double) * 6 * N);
  fclose(f);

  int32_t *steps = need(sizeof(int32_t) * 8 * S);
  difficulty_host_trav_steps(gt, 1, W, H, starts, S, steps);
  if (memcmp(steps, want_steps, sizeof(int32_t) * 8 * S)) return 4;
  free(steps);
  for (int s = 0; s < S; ++s) {   /* every start alone: S = 1 */
    int32_t *s1 = need(sizeof(int32_t) * 2), *o1 = need(sizeof(int32_t) * 8);
    memcpy(s1, starts + 2 * s, sizeof(int32_t) * 2);
    difficulty_host_trav_steps(gt, 1, W, H, s1, 1, o1);
    if (memcmp(o1, want_steps + 8 * s, sizeof(int32_t) * 8)) return 5;
    free(s1);
    free(o1);
  }

  double *end = need(sizeof(double) * 6 * N);
  int32_t *first = fit(ag, pos, N, P, checks, end);
  if (memcmp(first, want_first, sizeof(int32_t) * P) || memcmp(end, want_end, sizeof(double) * 6 * N)) return 6;
  free(first);
  free(end);
  first = fit(ag, pos, N, P, checks, NULL);   /* agents_out = NULL */
  if (memcmp(first, want_first, sizeof(int32_t) * P)) return 7;
  free(first);
  for (int p = 0; p < P; ++p) {   /* every position alone: P = 1 */
    double *p1 = need(sizeof(double) * 2);
    memcpy(p1, pos + 2 * p, sizeof(double) * 2);
    first = fit(ag, p1, N, 1, checks, NULL);
    if (first[0] != want_first[p]) return 8;
    free(first);
    free(p1);
  }
  double *a1 = need(sizeof(double) * 6), *e1 = need(sizeof(double) * 6);   /* the first agent alone: N = 1; no check at all */
  for (int r = 0; r < 6; ++r) a1[r] = ag[(size_t)r * N];
  free(fit(a1, pos, 1, P, checks, e1));
  difficulty_host_fit_first_hit(a1, pos, 10.0, 500.0, 500.0, 10.0, 0.1, 1, 1, 1, 0, (first = need(sizeof(int32_t))), e1, (end = need(sizeof(double) * 5)));
  if (first[0] != -1) return 9;
  free(first); free(end); free(a1); free(e1);
  free(hdr); free(gt); free(starts); free(want_steps); free(ag); free(pos); free(want_first); free(want_end);
  return 0;
}
