/* Stand-alone driver of csrc/render/d2d_render.h for the sanitizer run of tests/test_render_host_build.py: reads the records the test
 * wrote, runs the host loops on exactly sized heap arrays (every buffer ends with its last byte) and writes what came out.
 *   record 1 (raster): int32 cap, W, H, W_px, H_px, scale, downsample, count; cap items; W * H cells
 *                      -> the FNV-1a 64 digest of the frame, 8 bytes
 *   record 2 (list):   int32 N, P, traj_len, n_seeded, steps, has_vel, cap; double R, range, drone_radius; drone [8]; agents [6][N];
 *                      active [N]; vel [2][N] if has_vel; target [2]; pillars [P][3] int32; traj [traj_len][2]; star [20]
 *                      -> int32 count (-1: does not fit cap), then count items
 * Exit status 0: done; 1: usage / read error; 2: a host loop refused its arguments. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "render/d2d_render.h"

static void *take(FILE *f, size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
    fprintf(stderr, "short read\n");
    exit(1);
  }
  return p;
}

static uint64_t fnv(const uint8_t *p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 3) return 1;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int32_t records = 0;
  if (fread(&records, sizeof records, 1, f) != 1) return 1;
  for (int r = 0; r < records; ++r) {
    int32_t tag = 0;
    if (fread(&tag, sizeof tag, 1, f) != 1) return 1;
    if (tag == 1) {
      int32_t h[8];
      if (fread(h, sizeof h, 1, f) != 1) return 1;
      const int d = h[6], Wf = (h[3] + d - 1) / d, Hf = (h[4] + d - 1) / d;
      d2d_render_item *items = take(f, (size_t)h[0] * sizeof(d2d_render_item));
      uint8_t *cells = take(f, (size_t)h[1] * h[2]);
      int32_t *count = malloc(sizeof(int32_t));
      int16_t *bbox = malloc((size_t)h[0] * 4 * sizeof(int16_t));
      const size_t bytes = (size_t)Hf * Wf * 3;
      uint8_t *frame = malloc(bytes ? bytes : 1);
      if (!count || !bbox || !frame) return 1;
      *count = h[7];
      memset(frame, 0xAB, bytes);
      d2d_render_raster_call c = {items, count, cells, bbox, frame, 1, h[0], h[1], h[2], h[3], h[4], h[5], h[6]};
      if (d2d_render_raster_seq(&c) != 0) return 2;
      const uint64_t dg = fnv(frame, bytes);
      fwrite(&dg, sizeof dg, 1, o);
      free(items); free(cells); free(count); free(bbox); free(frame);
    } else if (tag == 2) {
      int32_t h[7];
      double s[3];
      if (fread(h, sizeof h, 1, f) != 1 || fread(s, sizeof s, 1, f) != 1) return 1;
      const size_t N = (size_t)h[0], P = (size_t)h[1], T = (size_t)h[2];
      double *drone = take(f, D2D_DF * 8), *agents = take(f, D2D_AF * N * 8);
      uint8_t *active = take(f, N);
      double *vel = h[5] ? take(f, 2 * N * 8) : NULL, *target = take(f, 16);
      int32_t *pillars = take(f, P * 12);
      double *traj = take(f, T * 16), *star = take(f, 160);
      d2d_render_src src = {drone, agents, active, vel, target, pillars, traj, star, 2, h[2], h[0], h[1], h[3], h[4], s[0], s[1], s[2]};
      d2d_render_item *items = malloc((size_t)h[6] * sizeof(d2d_render_item));
      if (!items) return 1;
      const int32_t count = d2d_render_list_seq(&src, h[6], items);
      fwrite(&count, sizeof count, 1, o);
      if (count > 0) fwrite(items, sizeof(d2d_render_item), (size_t)count, o);
      free(drone); free(agents); free(active); free(vel); free(target); free(pillars); free(traj); free(star); free(items);
    } else {
      return 1;
    }
  }
  fclose(f);
  fclose(o);
  return 0;
}
