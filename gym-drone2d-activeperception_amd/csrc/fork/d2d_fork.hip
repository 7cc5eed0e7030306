// d2d_fork.hip — the slot fork on the device (gfx950): the kernel + the C entry points of include/d2d_fork.h.  Its own library
// (libd2d_fork.so): it shares no kernel with the step, the closed loop, the planners, the observation channels or the world build.
//
//   fork_slots_kernel   D2D_FORK_PARTS workgroups of D2D_FORK_BLOCK threads (one wave) per destination slot, workgroup = slot * parts
//                       + part: the launch shape of stream_restore_kernel (csrc/worlds/d2d_worlds_turn.inc).
//                       gate   d2d_fork_decide: src_of[e] and, in place, src_of[src_of[e]], uniform over the workgroup.  A slot that
//                              is left or refused ends there; part 0 writes its status byte.
//                       copy   the item array is read from device memory, uniformly over the workgroup; what a thread copies for an
//                              item is d2d_fork_copy_row (d2d_fork.h), the text the host build checks under a sanitizer.  All stores
//                              are plain vector stores, 16 bytes a lane where source and destination agree modulo 16.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_FORK_QUAL __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define D2D_FORK_MEM __attribute__((address_space(1)))
#endif
#include "d2d_fork.h"

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

__global__ __launch_bounds__(D2D_FORK_BLOCK) void fork_slots_kernel(const d2d_fork_item *__restrict__ items, int n_items,
                                                                   const int32_t *__restrict__ src_of, int B_src, int in_place,
                                                                   uint8_t *__restrict__ status) {
  const int64_t e = (int64_t)(blockIdx.x / D2D_FORK_PARTS);  // < B_dst: the grid is B_dst * parts
  const int part = (int)(blockIdx.x % D2D_FORK_PARTS);
  const int st = d2d_fork_decide(src_of, e, B_src, in_place);
  if (part == 0 && threadIdx.x == 0) status[e] = (uint8_t)st;
  if (st != D2D_FORK_COPIED) return;
  const int64_t s = (int64_t)src_of[e];  // in [0, B_src)
  for (int k = 0; k < n_items; ++k) d2d_fork_copy_row(items + k, k, e, s, part, (int)threadIdx.x, D2D_FORK_BLOCK);
}

}  // namespace

extern "C" {

int d2d_fork_version(void) { return D2D_FORK_VERSION; }
const char *d2d_fork_last_error(void) { return g_err; }

int d2d_fork_slots(const d2d_fork_item *items, int32_t n_items, const int32_t *src_of, int32_t B_dst, int32_t B_src, int32_t in_place,
                   uint8_t *status, void *stream) {
  const char *why;
  const int rc = d2d_fork_check(items, n_items, src_of, B_dst, B_src, in_place, status, &why);
  if (rc) return fail(rc, why);
  if (B_dst == 0) return 0;
  hipLaunchKernelGGL(fork_slots_kernel, dim3((unsigned)B_dst * D2D_FORK_PARTS), dim3(D2D_FORK_BLOCK), 0, (hipStream_t)stream, items,
                     (int)n_items, src_of, (int)B_src, in_place != 0, status);
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "d2d_fork_slots: launch failed: %s", hipGetErrorString(err));
  return -3;
}

}  // extern "C"
