/* Stand-alone driver of tests/csrc/tracks_host.c for the sanitizer run of tests/test_tracks_obs_cpu.py: reads the records the test
 * wrote (one handmade set each: sizes, inputs, the poisoned outputs, then the answers the numpy model gave without and with `force`),
 * runs the host loop on exactly sized heap arrays -- twice without force (the second call must change nothing), once with -- and
 * compares byte for byte.  Exit status 0: every record equal; 1: usage / read error; 2: an answer differs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "tracks/d2d_tracks.h"

int tracks_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_tracks *tracks);

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
    double s[4];
    if (fread(h, sizeof h, 1, f) != 1 || fread(s, sizeof s, 1, f) != 1) return 1;
    const size_t B = (size_t)h[0], N = (size_t)h[1], LL = (size_t)h[4] * (size_t)h[4];
    double *drone = take(f, B * D2D_DF * 8);
    int32_t *counters = take(f, B * D2D_CF * 4);
    double *kf = take(f, B * N * D2D_KF * 8);
    uint8_t *active = take(f, B * N);
    double *radius = take(f, B * N * 8);
    uint8_t *win = take(f, B * LL);
    int32_t *cells = take(f, B * 4), *last = take(f, B * 4);
    uint8_t *want_win[2];
    int32_t *want_cells[2], *want_last[2];
    for (int v = 0; v < 2; ++v) {
      want_win[v] = take(f, B * LL);
      want_cells[v] = take(f, B * 4);
      want_last[v] = take(f, B * 4);
    }
    d2d_cfg c;
    d2d_state st;
    memset(&c, 0, sizeof c);
    memset(&st, 0, sizeof st);
    c.abi_version = D2D_ABI_VERSION;
    c.B = h[0]; c.N = h[1]; c.W = h[2]; c.H = h[3]; c.L = h[4];
    c.scale = s[0]; c.dt = s[1]; c.drone_radius = s[2];
    st.drone = drone;
    st.counters = counters;
    st.kf = kf;
    st.active = active;
    d2d_tracks w = {radius, win, cells, last, s[3], h[5], 0};
    for (int pass = 0; pass < 3; ++pass) {
      const int v = pass == 2;
      w.force = v;
      if (tracks_host_update(&c, &st, &w) != 0) return 2;
      if (memcmp(win, want_win[v], B * LL) || memcmp(cells, want_cells[v], B * 4) || memcmp(last, want_last[v], B * 4)) {
        fprintf(stderr, "record %d differs in pass %d\n", r, pass);
        return 2;
      }
    }
    free(drone); free(counters); free(kf); free(active); free(radius); free(win); free(cells); free(last);
    for (int v = 0; v < 2; ++v) {
      free(want_win[v]); free(want_cells[v]); free(want_last[v]);
    }
  }
  fclose(f);
  return 0;
}
