// d2d_tracks.hip — the tracker-forecast map as an observation channel on the device (gfx950): the kernel + the C entry points of
// include/d2d_tracks.h.  Its own library (libd2d_tracks.so): it shares no kernel with the step, the closed loop, the planners or
// the other observation channels.
//
//   tracks_update   one wave per env, up to four envs a workgroup, each wave with its own slice of LDS.
//                   gate       the env's step counter and the counter of its latest update are requested together: an env that is
//                              not due (finished, or updated already) ends there and writes nothing.
//                   stage      the active trackers into LDS, 64 a pass, compacted with a ballot as k_swept_mark does it: mu,
//                              velocity, the threshold and its squared form.  The window plane (32 bits a cell) is set to "none".
//                   rasterise  lane = (tracker, sample) pair, 64 pairs a pass: the forecast, the bounding box of its disc inside
//                              the window with one cell of slack, the exact test on every cell of the box, and an LDS atomicMin of
//                              k + 1.  A minimum: every order gives the same bytes.
//                   write      the finished window goes out whole as bytes, which is also what clears it; the nonzero cells are
//                              counted by ballots; lane 0 writes cells and last_step.
//
// Arithmetic is fp64 in the reference's own operation order (d2d_tracks.h), compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_TRACKS_QUAL __device__ __forceinline__
#include "d2d_tracks.h"

#define WAVE 64
#define TRACKS_WAVES 4

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

extern __shared__ __attribute__((aligned(16))) unsigned char tracks_lds[];

// the wave's own LDS writes are complete and visible to its own reads (no other wave touches its slice)
__device__ __forceinline__ void wave_sync_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(TRACKS_WAVES *WAVE) void tracks_update_kernel(const d2d_cfg c, const double *__restrict__ drone,
                                                                          const int32_t *__restrict__ counters,
                                                                          const uint8_t *__restrict__ active,
                                                                          const double *__restrict__ kf, const d2d_tracks w,
                                                                          const unsigned wave_bytes) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long e = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
  if (e >= c.B) return;

  // ---- gate: one batch of loads ----
  const int steps = counters[(size_t)e * D2D_CF + D2D_C_STEPS];
  const int last = w.last_step[e];
  const double *dr = drone + (size_t)e * D2D_DF;
  const double x0 = dr[D2D_D_X], y0 = dr[D2D_D_Y];
  if (!d2d_tracks_due(steps, last, w.force)) return;

  const int N = c.N, W = c.W, H = c.H, L = c.L, edge = (L - 1) / 2, nn = L * L;
  const size_t NP = (size_t)(N > 0 ? N : 1);
  unsigned char *base = tracks_lds + (size_t)wv * wave_bytes;
  double *tmx = (double *)base, *tmy = tmx + NP, *tvx = tmy + NP, *tvy = tvx + NP, *tthr = tvy + NP, *tlim = tthr + NP;
  uint32_t *plane = (uint32_t *)(base + ((NP * 6 * sizeof(double) + 15) & ~(size_t)15));  // (d2d_tracks_wave_bytes)
  for (int a = lane; a < nn; a += WAVE) plane[a] = D2D_TRACKS_NONE;

  // ---- stage: the active trackers, compacted.  q < nact <= N: inside the planes ----
  int nact = 0;
  for (int k0 = 0; k0 < N; k0 += WAVE) {
    const int k = k0 + lane;
    bool act = false;
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, thr = 0, lim = -1.0;
    if (k < N) {
      const double *mu = kf + ((size_t)e * N + k) * D2D_KF;
      m0 = mu[0]; m1 = mu[1]; m2 = mu[2]; m3 = mu[3];
      act = active[(size_t)e * N + k] != 0;
      thr = c.drone_radius + w.trk_radius[(size_t)e * N + k] + w.margin;
      if (act) lim = d2d_tracks_sq_threshold(thr);
      act = act && lim >= 0.0;  // (a negative or NaN threshold: nothing is within it)
    }
    const unsigned long long am = __ballot(act);
    if (act) {
      const int q = nact + __popcll(am & ((1ull << lane) - 1ull));
      tmx[q] = m0; tmy[q] = m1; tvx[q] = m2; tvy[q] = m3; tthr[q] = thr; tlim[q] = lim;
    }
    nact += __popcll(am);
  }
  wave_sync_lds();

  // ---- rasterise: lane = (tracker, sample) ----
  const int i0 = d2d_tracks_cell(x0, c.scale, W) - edge, j0 = d2d_tracks_cell(y0, c.scale, H) - edge;
  const int samples = w.samples, npair = nact * samples;  // (at most N * 255)
  for (int p0 = 0; p0 < npair; p0 += WAVE) {
    const int pi = p0 + lane;
    if (pi < npair) {
      const int q = pi / samples, k = pi - q * samples;  // q in [0, nact)
      const double t = (double)k * c.dt, thr = tthr[q], lim = tlim[q];
      const double ex = d2d_tracks_estimate(tmx[q], tvx[q], t), ey = d2d_tracks_estimate(tmy[q], tvy[q], t);
      int i_lo, i_hi, j_lo, j_hi;
      d2d_tracks_span(ex, thr, c.scale, W, i0, L, &i_lo, &i_hi);  // i in [max(i0, 0), min(i0 + L, W) - 1]: i - i0 in [0, L)
      d2d_tracks_span(ey, thr, c.scale, H, j0, L, &j_lo, &j_hi);
      for (int i = i_lo; i <= i_hi; ++i) {
        const double dx = d2d_tracks_centre(i, c.scale) - ex, dx2 = dx * dx;
        const int row = (i - i0) * L - j0;  // row + j in [0, L * L)
        for (int j = j_lo; j <= j_hi; ++j) {
          const double dy = d2d_tracks_centre(j, c.scale) - ey;
          if (D2D_FMA(dy, dy, dx2) <= lim) atomicMin(plane + (row + j), (uint32_t)(k + 1));  // (d2d_tracks_hit, dx * dx taken out of the loop)
        }
      }
    }
  }
  wave_sync_lds();

  // ---- write: the window whole ----
  uint8_t *__restrict__ out = w.win + (size_t)e * nn;
  int cells = 0;
  for (int a0 = 0; a0 < nn; a0 += WAVE) {
    const int a = a0 + lane;
    bool on = false;
    if (a < nn) {
      const uint32_t v = plane[a];
      on = v < D2D_TRACKS_NONE;
      out[a] = (uint8_t)(on ? v : 0u);
    }
    cells += __popcll(__ballot(on));
  }
  if (lane == 0) {
    w.cells[e] = cells;
    w.last_step[e] = steps;
  }
}

}  // namespace

extern "C" {

int d2d_tracks_version(void) { return D2D_TRACKS_VERSION; }
const char *d2d_tracks_last_error(void) { return g_err; }

int d2d_tracks_update(const d2d_cfg *c, const d2d_state *s, const d2d_tracks *w, void *stream) {
  const char *why;
  const int rc = d2d_tracks_check(c, s, w, &why);
  if (rc) return fail(rc, why);
  if (c->B == 0) return 0;
  const size_t wb = d2d_tracks_wave_bytes(c->N, c->L);
  int wpb = (int)(D2D_TRACKS_LDS_BYTES / wb);  // (>= 1: checked)
  if (wpb > TRACKS_WAVES) wpb = TRACKS_WAVES;
  hipLaunchKernelGGL(tracks_update_kernel, dim3((unsigned)(((long long)c->B + wpb - 1) / wpb)), dim3(wpb * WAVE), wb * wpb,
                     (hipStream_t)stream, *c, (const double *)s->drone, (const int32_t *)s->counters, (const uint8_t *)s->active,
                     (const double *)s->kf, *w, (unsigned)wb);
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "d2d_tracks_update: launch failed: %s", hipGetErrorString(err));
  return -3;
}

}  // extern "C"
