/* Host build of the step path's gaze arithmetic (csrc/gaze/d2d_gaze.h) for tests/test_gaze_host_build.py and tests/gaze_backend.py:
 * the two entry points of include/d2d_gaze.h as loops over host arrays, and the scalar pieces the tests look at on their own. */
#include <math.h>
#include <stdint.h>
#include "d2d_gaze.h"
int gaze_host_act(const d2d_gaze_call *call) { return d2d_gaze_act_seq(call); }
int gaze_host_reset(double *owl_state, const uint8_t *mask, int32_t mask_stride, int32_t B) {
  return d2d_gaze_reset_seq(owl_state, mask, mask_stride, B);
}
double gaze_host_mod360(double a) { return d2d_gaze_mod360(a); }
double gaze_host_lookahead(double vx, double vy, double yaw, double dt, double w) { return d2d_gaze_lookahead(vx, vy, yaw, dt, w); }
int gaze_host_version(void) { return D2D_GAZE_VERSION; }
int gaze_host_call_bytes(void) { return (int)sizeof(d2d_gaze_call); }
int gaze_host_offsets(int32_t *out) { /* the owl_tab offsets and limits this build was compiled with */
  const int32_t v[] = {D2D_GAZE_T_RATE, D2D_GAZE_T_RATE08, D2D_GAZE_T_TURN, D2D_GAZE_T_ACT, D2D_GAZE_T_DIR, D2D_GAZE_T_FOV,
                       D2D_GAZE_T_DEPTH, D2D_GAZE_T_HOLD, D2D_GAZE_OWL_TAB_LEN, D2D_GAZE_OWL_STATE_F, D2D_GAZE_OWL_S_RATE,
                       D2D_GAZE_OWL_S_LEFT, D2D_GAZE_NRATE, D2D_GAZE_NDIR, D2D_GAZE_MAX_N, D2D_GAZE_K_LOOKAHEAD, D2D_GAZE_K_OWL,
                       D2D_GAZE_F_DONE, D2D_GAZE_DF, D2D_GAZE_KF};
  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
  return (int)(sizeof v / sizeof v[0]);
}
