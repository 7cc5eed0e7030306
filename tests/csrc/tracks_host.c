/* Host build of the tracker-forecast map's arithmetic (csrc/tracks/d2d_tracks.h) for tests/test_tracks_obs_cpu.py: the entry point of
 * include/d2d_tracks.h as a loop over host arrays, and the sizes the ctypes mirror is checked against. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "tracks/d2d_tracks.h"
int tracks_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_tracks *tracks) {
  if (!cfg || cfg->L < 1 || (long long)cfg->L * cfg->L > 0x7fffffffll) return d2d_tracks_update_seq(cfg, st, tracks, NULL);
  uint32_t *plane = (uint32_t *)malloc((size_t)cfg->L * cfg->L * sizeof(uint32_t)); /* exactly sized: the window's own indices */
  const int rc = d2d_tracks_update_seq(cfg, st, tracks, plane);
  free(plane);
  return rc;
}
int tracks_host_check(const d2d_cfg *cfg, const d2d_state *st, const d2d_tracks *tracks, char *why, int n) {
  const char *text;
  const int rc = d2d_tracks_check(cfg, st, tracks, &text);
  int i = 0;
  for (; i + 1 < n && text[i]; ++i) why[i] = text[i];
  if (n > 0) why[i] = 0;
  return rc;
}
int tracks_host_version(void) { return D2D_TRACKS_VERSION; }
int tracks_host_struct_bytes(void) { return (int)sizeof(d2d_tracks); }
int tracks_host_cell(double v, double s, int limit) { return d2d_tracks_cell(v, s, limit); }
double tracks_host_sq_threshold(double r) { return d2d_tracks_sq_threshold(r); }
