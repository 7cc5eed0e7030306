/* Stand-alone program around the redraw's scalar statement and the sequential world build with D2D_WE_REDRAW set, for a run under
 * AddressSanitizer / UBSan (tests/test_validation_redraw_cpu.py builds it with host_build.sanitized and runs it as a child process).
 * Prints a checksum of the redrawn velocities of a few worlds; exit status 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "worlds/d2d_worlds.h"

int main(void) {
  enum { B = 3, NR = 70, W = 50, H = 50 };
  d2d_world_spec s;
  d2d_state st;
  memset(&s, 0, sizeof s);
  memset(&st, 0, sizeof st);
  s.version = D2D_WORLDS_VERSION; s.B = B; s.N = NR; s.n_rand = NR; s.T = 1; s.W_px = 500; s.H_px = 500; s.scale = 10; s.W = W; s.H = H;
  s.max_attempts = D2D_WORLDS_MAX_ATTEMPTS; s.start_clear = 80.0; s.pillar_clear = 30.0;
  double *unit = calloc(2 * NR, sizeof(double)), *par = calloc(B * D2D_WORLDS_ENV_F, sizeof(double)), *tgt = calloc(B * 2, sizeof(double));
  uint32_t map_id[B] = {0, 1, 4294967295u};
  double *trk = calloc(B * NR, sizeof(double));
  int32_t status[B];
  for (int e = 0; e < B; ++e) {
    double *p = par + e * D2D_WORLDS_ENV_F;
    p[D2D_WE_R_LO] = 3.0; p[D2D_WE_R_W] = 4.0; p[D2D_WE_SPEED] = 40.0; p[D2D_WE_TRK_R] = 5.0; p[D2D_WE_X0] = 50.0; p[D2D_WE_Y0] = 50.0;
    p[D2D_WE_NTGT] = 1.0; p[D2D_WE_REDRAW] = e == 1 ? 0.0 : 1.0;
    tgt[2 * e] = 50.0; tgt[2 * e + 1] = 460.0;
  }
  s.unit = unit; s.map_id = map_id; s.env_par = par; s.env_tgt = tgt; s.tracker_radius = trk; s.status = status;
  st.agents = calloc(B * D2D_AF * NR, sizeof(double)); st.agent_unit = calloc(B * NR, sizeof(int32_t));
  st.dyn_prev = calloc(B * NR * 3, sizeof(int32_t)); st.gt = calloc(B * W * H, 1); st.dmap = calloc(B * W * H, 1);
  st.drone = calloc(B * D2D_DF, sizeof(double)); st.target = calloc(B * 2, sizeof(double)); st.targets = calloc(B * 2, sizeof(double));
  st.counters = calloc(B * D2D_CF, sizeof(int32_t)); st.active = calloc(B * NR, 1);
  uint32_t *buf = malloc(sizeof(uint32_t) * D2D_W_BUF);
  double *acc = malloc(sizeof(double) * D2D_W_ACC_F * (NR + 1));
  double sum = 0.0;
  for (int e = 0; e < B; ++e) {
    d2d_worlds_build_seq_env(&s, &st, e, buf, acc);
    for (int k = 0; k < NR; ++k) sum += st.agents[(e * D2D_AF + D2D_A_VX) * NR + k] + st.agents[(e * D2D_AF + D2D_A_VY) * NR + k];
  }
  printf("%d %d %d %.17g\n", status[0], status[1], status[2], sum);
  free(unit); free(par); free(tgt); free(trk); free(st.agents); free(st.agent_unit); free(st.dyn_prev); free(st.gt); free(st.dmap);
  free(st.drone); free(st.target); free(st.targets); free(st.counters); free(st.active); free(buf); free(acc);
  return 0;
}
