/* Stand-alone driver of tests/csrc/gaze_host.c for the sanitizer run of tests/test_gaze_host_build.py: reads the records the test
 * wrote (one d2d_gaze_act call each: inputs, then the answers the host policies gave), runs the host loop on exactly sized heap arrays
 * and compares byte for byte.  Exit status 0: every record equal; 1: usage / read error; 2: an answer differs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "d2d_gaze.h"

int gaze_host_act(const d2d_gaze_call *call);
int gaze_host_reset(double *owl_state, const uint8_t *mask, int32_t mask_stride, int32_t B);

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
    int32_t h[4];
    double s[2];
    if (fread(h, sizeof h, 1, f) != 1 || fread(s, sizeof s, 1, f) != 1) return 1;
    const size_t B = (size_t)h[0], N = (size_t)h[1];
    double *drone = take(f, B * D2D_GAZE_DF * 8), *target = take(f, B * 2 * 8);
    uint8_t *active = take(f, B * N);
    double *kf = take(f, B * N * D2D_GAZE_KF * 8);
    uint8_t *flags = take(f, B * 4);
    double *owl = take(f, B * D2D_GAZE_OWL_STATE_F * 8), *tab = take(f, D2D_GAZE_OWL_TAB_LEN * 8), *action = take(f, B * 8);
    double *want_a = take(f, B * 8), *want_o = take(f, B * D2D_GAZE_OWL_STATE_F * 8);
    d2d_gaze_call c = {drone, target, N ? active : NULL, N ? kf : NULL, h[3] ? flags : NULL, owl, tab, action,
                       h[0], h[1], h[2], 0, s[0], s[1]};
    if (gaze_host_act(&c) != 0) return 2;
    if (memcmp(action, want_a, B * 8) || memcmp(owl, want_o, B * D2D_GAZE_OWL_STATE_F * 8)) {
      fprintf(stderr, "record %d differs\n", r);
      return 2;
    }
    /* the reset: the envs of a mask, then all */
    uint8_t *mask = calloc(B, 1);
    for (size_t b = 0; b < B; b += 2) mask[b] = 1;
    if (gaze_host_reset(owl, mask, 1, (int32_t)B) != 0) return 2;
    for (size_t b = 0; b < B; ++b)
      for (int k = 0; k < D2D_GAZE_OWL_STATE_F; ++k) {
        const double got = owl[b * D2D_GAZE_OWL_STATE_F + k], was = want_o[b * D2D_GAZE_OWL_STATE_F + k];
        if (mask[b] ? (got != 0.0) : memcmp(&got, &was, 8) != 0) return 2;
      }
    if (gaze_host_reset(owl, NULL, 1, (int32_t)B) != 0) return 2;
    for (size_t i = 0; i < B * D2D_GAZE_OWL_STATE_F; ++i)
      if (owl[i] != 0.0) return 2;
    free(mask); free(drone); free(target); free(active); free(kf); free(flags); free(owl); free(tab); free(action); free(want_a); free(want_o);
  }
  fclose(f);
  return 0;
}
