/* Stand-alone sanitizer target of tests/test_rvo_host_build.py: the host loops of csrc/rvo/d2d_rvo.h (through rvo_host.c) on exactly
 * sized heap arrays.  argv[1] is a case file the test writes: int32 count, then per scene int32 N, P, doubles agents [6][N],
 * vel [2][N], int32 pillars [P][3], and what the Python model expects: doubles vel_out [2][N], agents_end [6][N].  Every scene runs
 * whole (results compared).  Built with -fsanitize=address,undefined; exits 0 and writes nothing to stderr. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int rvo_host_velocity(const double *, const double *, const int32_t *, int32_t, int32_t, int32_t, double *, double *);
void rvo_host_agents_step(double *, const double *, double, double, double, double, int32_t, int32_t);

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
    int32_t *hdr = take(f, sizeof(int32_t) * 2);
    const int N = hdr[0], P = hdr[1];
    if (N < 0 || P < 0) return 66;
    const size_t nc = N > 0 ? (size_t)(N - 1 + P) : 0;
    double *ag = take(f, sizeof(double) * 6 * N), *vel = take(f, sizeof(double) * 2 * N);
    int32_t *pil = take(f, sizeof(int32_t) * 3 * P);
    double *want_vel = take(f, sizeof(double) * 2 * N), *want_ag = take(f, sizeof(double) * 6 * N);
    double *out = need(sizeof(double) * 2 * N), *work = need(sizeof(double) * 6 * nc);
    if (rvo_host_velocity(ag, vel, pil, 1, N, P, out, work)) return 3;
    if (memcmp(out, want_vel, sizeof(double) * 2 * N)) return 4;
    rvo_host_agents_step(ag, out, 500.0, 500.0, 10.0, 0.1, 1, N);
    if (memcmp(ag, want_ag, sizeof(double) * 6 * N)) return 5;
    free(hdr); free(ag); free(vel); free(pil); free(want_vel); free(want_ag); free(out); free(work);
  }
  fclose(f);
  free(count);
  return 0;
}
