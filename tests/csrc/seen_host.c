/* Host build of the time-since-observed map's arithmetic (csrc/seen/d2d_seen.h) for tests/test_seen_obs_cpu.py: the entry point of
 * include/d2d_seen.h as a loop over host arrays, and the sizes the ctypes mirror is checked against. */
#include <math.h>
#include <stdint.h>
#include "seen/d2d_seen.h"
int seen_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_seen *seen) { return d2d_seen_update_seq(cfg, st, seen); }
int seen_host_check(const d2d_cfg *cfg, const d2d_state *st, const d2d_seen *seen, char *why, int n) {
  const char *text;
  const int rc = d2d_seen_check(cfg, st, seen, &text);
  int i = 0;
  for (; i + 1 < n && text[i]; ++i) why[i] = text[i];
  if (n > 0) why[i] = 0;
  return rc;
}
int seen_host_version(void) { return D2D_SEEN_VERSION; }
int seen_host_struct_bytes(void) { return (int)sizeof(d2d_seen); }
int seen_host_cell(double v, double s, int limit) { return d2d_seen_cell(v, s, limit); }
