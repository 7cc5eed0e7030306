/*
 * d2d_hooks.h — test hooks of the HIP library (libd2d_hip.so) alone.
 *
 * include/d2d.h is the surface both implementations export (the CPU oracle as d2d_oracle_*); the entry points
 * here exist only where there is a device restatement to check, so they stay out of that shared surface.
 */
#ifndef D2D_HOOKS_H
#define D2D_HOOKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device restatement of Python's math.atan2 (CPython's special cases over the host libm atan2) that the LookAhead and
 * LookGoal gaze stages call (yaw_planner.py:33, :251): out[i] = atan2(y[i], x[i]), bit-for-bit glibc 2.35 x86-64
 * FMA variant.  Returns 0, or a negative error like every entry point. */
int d2d_atan2_array(const double *y, const double *x, double *out, int64_t n, void *stream);

/* Device restatement of the host libm pow(x, 2.0) that numpy's `float64 ** 2` resolves to in the Owl gaze stage
 * (yaw_planner.py:209): out[i] = pow(x[i], 2.0), bit-for-bit glibc 2.35 x86-64 FMA variant (not x * x).  Returns 0, or a
 * negative error like every entry point. */
int d2d_pow2_array(const double *x, double *out, int64_t n, void *stream);

/* Device restatement of the host libm log that numpy's legacy Gaussian calls for the measurement noise (utils.py:605):
 * out[i] = log(x[i]), bit-for-bit glibc 2.35 x86-64 FMA variant.  Returns 0, or a negative error like every entry point. */
int d2d_log_array(const double *x, double *out, int64_t n, void *stream);

/* The measurement noise's random stream on its own: draws m[b] pairs (np.random.randn(2) each) from stream b of
 * rng [B][D2D_RNG_WORDS] into out[b][k][0..1], k < m[b] <= max_m (the rest of out[b] is set to 0), and advances the stream, as the
 * tracker stage does for the m[b] agents in view (include/d2d.h, d2d_state.rng).  Returns 0, or a negative error like every
 * entry point. */
int d2d_rng_draw(uint32_t *rng, const int32_t *m, double *out, int32_t B, int32_t max_m, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_HOOKS_H */
