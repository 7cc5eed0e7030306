/* Host build of the per-ray scan's arithmetic (csrc/scan/d2d_scan.h) for tests/test_scan_obs_cpu.py: the entry point of
 * include/d2d_scan.h as a loop over host arrays, and the sizes the ctypes mirror is checked against. */
#include <math.h>
#include <stdint.h>
#include "scan/d2d_scan.h"
int scan_host_update(const d2d_cfg *cfg, const d2d_state *st, const d2d_scan *scan) { return d2d_scan_update_seq(cfg, st, scan); }
int scan_host_check(const d2d_cfg *cfg, const d2d_state *st, const d2d_scan *scan, char *why, int n) {
  const char *text;
  const int rc = d2d_scan_check(cfg, st, scan, &text);
  int i = 0;
  for (; i + 1 < n && text[i]; ++i) why[i] = text[i];
  if (n > 0) why[i] = 0;
  return rc;
}
int scan_host_version(void) { return D2D_SCAN_VERSION; }
int scan_host_struct_bytes(void) { return (int)sizeof(d2d_scan); }
int scan_host_cell(double v, double s, int n) { return d2d_scan_cell(v, s, n); }
double scan_host_positive_angle(double a) { return d2d_scan_positive_angle(a); }
