/* Stand-alone driver of tests/csrc/seen_host.c for the sanitizer run of tests/test_seen_obs_cpu.py: reads the records the test wrote
 * (one d2d_seen_update call each: sizes, inputs, then the answers the numpy model gave), runs the host loop on exactly sized heap
 * arrays, twice (the second call must change nothing), and compares byte for byte.  Exit status 0: every record equal; 1: usage /
 * read error; 2: an answer differs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "seen/d2d_seen.h"

int seen_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_seen *seen);

static void *take(FILE *f, size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
    fprintf(stderr, "short read\n");
    exit(1);
  }
  return p;
}

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t count = 0;
  if (fread(&count, sizeof count, 1, f) != 1) return 1;
  for (int r = 0; r < count; ++r) {
    int32_t h[6];
    double s[2];
    int64_t key_lo;
    uint64_t mask;
    if (fread(h, sizeof h, 1, f) != 1 || fread(s, sizeof s, 1, f) != 1 || fread(&key_lo, 8, 1, f) != 1 || fread(&mask, 8, 1, f) != 1) return 1;
    const size_t B = (size_t)h[0], WH = (size_t)h[1] * (size_t)h[2], LL = (size_t)h[3] * (size_t)h[3], n = (size_t)h[4];
    double *drone = take(f, B * D2D_DF * 8);
    int32_t *counters = take(f, B * D2D_CF * 4), *seen = take(f, B * WH * 4), *last = take(f, B * 4), *refreshed = take(f, B * 4);
    float *obs = take(f, B * LL * 4);
    double *tab = take(f, 2 * n * 8);
    int32_t *want_seen = take(f, B * WH * 4), *want_last = take(f, B * 4), *want_refreshed = take(f, B * 4);
    float *want_obs = take(f, B * LL * 4);
    d2d_cfg c;
    d2d_state st;
    memset(&c, 0, sizeof c);
    memset(&st, 0, sizeof st);
    c.abi_version = D2D_ABI_VERSION;
    c.B = h[0]; c.W = h[1]; c.H = h[2]; c.L = h[3];
    c.scale = s[0]; c.depth = s[1];
    st.drone = drone;
    st.counters = counters;
    d2d_seen w = {seen, last, refreshed, obs, tab, key_lo, mask, h[4], 0};
    for (int pass = 0; pass < 2; ++pass) {
      if (seen_host_update(&c, &st, &w) != 0) return 2;
      if (memcmp(seen, want_seen, B * WH * 4) || memcmp(last, want_last, B * 4) || memcmp(refreshed, want_refreshed, B * 4) ||
          memcmp(obs, want_obs, B * LL * 4)) {
        fprintf(stderr, "record %d differs in pass %d\n", r, pass);
        return 2;
      }
    }
    free(drone); free(counters); free(seen); free(last); free(refreshed); free(obs); free(tab);
    free(want_seen); free(want_last); free(want_refreshed); free(want_obs);
  }
  fclose(f);
  return 0;
}
