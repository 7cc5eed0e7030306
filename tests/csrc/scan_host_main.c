/* Stand-alone driver of tests/csrc/scan_host.c for the sanitizer run of tests/test_scan_obs_cpu.py: reads the records the test wrote
 * (one d2d_scan_update call each: sizes, inputs, the buffers as they were before the call, then the answers the Python model gave),
 * runs the host loop on exactly sized heap arrays, twice (the second call must change nothing), and compares byte for byte.  Exit
 * status 0: every record equal; 1: usage / read error; 2: an answer differs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scan/d2d_scan.h"

int scan_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_scan *scan);

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
    int32_t h[8];  /* B, N, W, H, R, grid_tile, hit_words, 0 */
    double s[6];   /* scale, W_px, H_px, ray_off0, ray_dth, depth */
    if (fread(h, sizeof h, 1, f) != 1 || fread(s, sizeof s, 1, f) != 1) return 1;
    d2d_cfg c;
    d2d_state st;
    memset(&c, 0, sizeof c);
    memset(&st, 0, sizeof st);
    c.abi_version = D2D_ABI_VERSION;
    c.B = h[0]; c.N = h[1]; c.W = h[2]; c.H = h[3]; c.R = h[4]; c.grid_tile = h[5];
    c.scale = s[0]; c.W_px = s[1]; c.H_px = s[2]; c.ray_off0 = s[3]; c.ray_dth = s[4]; c.depth = s[5];
    const size_t B = (size_t)h[0], N = (size_t)h[1], R = (size_t)h[4], hw = (size_t)h[6], gb = D2D_GRID_BYTES(&c);
    double *agents = take(f, B * D2D_AF * N * 8);
    int32_t *counters = take(f, B * D2D_CF * 4);
    uint8_t *gt = take(f, B * gb);
    double *pose = take(f, B * D2D_DF * 8), *end = take(f, B * R * 2 * 8);
    uint8_t *kind = take(f, B * R);
    uint32_t *hit = take(f, B * R * hw * 4);
    float *obs = take(f, B * 2 * R * 4);
    int32_t *last = take(f, B * 4);
    double *want_end = take(f, B * R * 2 * 8);
    uint8_t *want_kind = take(f, B * R);
    uint32_t *want_hit = take(f, B * R * hw * 4);
    float *want_obs = take(f, B * 2 * R * 4);
    int32_t *want_last = take(f, B * 4);
    st.agents = agents;
    st.counters = counters;
    st.gt = gt;
    d2d_scan w = {pose, end, kind, hit, obs, last, h[6], 0};
    for (int pass = 0; pass < 2; ++pass) {
      if (scan_host_update(&c, &st, &w) != 0) return 2;
      if (memcmp(end, want_end, B * R * 16) || memcmp(kind, want_kind, B * R) || memcmp(hit, want_hit, B * R * hw * 4) ||
          memcmp(obs, want_obs, B * 2 * R * 4) || memcmp(last, want_last, B * 4)) {
        fprintf(stderr, "record %d differs in pass %d\n", r, pass);
        return 2;
      }
    }
    free(agents); free(counters); free(gt); free(pose); free(end); free(kind); free(hit); free(obs); free(last);
    free(want_end); free(want_kind); free(want_hit); free(want_obs); free(want_last);
  }
  fclose(f);
  return 0;
}
