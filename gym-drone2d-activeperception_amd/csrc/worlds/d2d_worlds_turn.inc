// d2d_worlds_turn.inc -- the kernels and entry points of include/d2d_worlds_turn.h, the tail of d2d_worlds.hip (it uses that file's
// fail(), launched(), wave_sum() and nonzero_bytes()).
//
//   stream_restore_kernel   D2D_RESTORE_PARTS workgroups of D2D_RESTORE_BLOCK threads per slot, workgroup = slot * parts + part.  The
//                           item array is read from device memory, uniformly over the workgroup; what a thread writes for an item is
//                           d2d_restore_apply (d2d_restore.h), the text the host build checks under a sanitizer.  All stores are
//                           plain vector stores.
//   stream_explored_kernel  one wave per slot, the count of d2d_stream_count.inc.

namespace {

__global__ __launch_bounds__(D2D_RESTORE_BLOCK) void stream_restore_kernel(const d2d_restore_item *items, int n_items, const uint8_t *refill) {
  const unsigned e = blockIdx.x / D2D_RESTORE_PARTS;
  if (!refill[e]) return;
  const int part = (int)(blockIdx.x % D2D_RESTORE_PARTS);
  for (int k = 0; k < n_items; ++k) d2d_restore_apply(items + k, k, (int64_t)e, part, (int)threadIdx.x, D2D_RESTORE_BLOCK);
}

__global__ __launch_bounds__(WAVE) void stream_explored_kernel(const d2d_state st, int W, int H, int tile, int32_t *cells) {
  const int e = blockIdx.x, lane = threadIdx.x;
#include "d2d_stream_count.inc"
  if (lane == 0) cells[e] = cnt;
}

}  // namespace

extern "C" {

int d2d_stream_restore(const d2d_restore_item *items, int32_t n_items, const uint8_t *refill, int32_t B, void *stream) {
  if (B < 0 || n_items < 0 || n_items > D2D_RESTORE_MAX_ITEMS)
    return fail(-1, "d2d_stream_restore: B >= 0, 0 <= n_items <= D2D_RESTORE_MAX_ITEMS");
  if ((long long)B * D2D_RESTORE_PARTS > 0x7fffffffLL) return fail(-4, "d2d_stream_restore: B * D2D_RESTORE_PARTS workgroups exceed the grid");
  if (B == 0 || n_items == 0) return 0;
  if (!items || !refill) return fail(-1, "d2d_stream_restore: a pointer is NULL");
  if ((uintptr_t)items & 7u) return fail(-1, "d2d_stream_restore: items aligned to 8 bytes");
  hipLaunchKernelGGL(stream_restore_kernel, dim3((unsigned)B * D2D_RESTORE_PARTS), dim3(D2D_RESTORE_BLOCK), 0, (hipStream_t)stream, items,
                     (int)n_items, refill);
  return launched();
}

int d2d_stream_explored(const d2d_state *st, int32_t B, int32_t W, int32_t H, int32_t grid_tile, int32_t *cells, void *stream) {
  if (B < 0 || W < 1 || H < 1) return fail(-1, "d2d_stream_explored: B >= 0, W, H >= 1");
  if (grid_tile != 0 && grid_tile != 16) return fail(-1, "d2d_stream_explored: grid_tile is 0 or 16");
  if (((long long)(W + 15) / 16) * ((H + 15) / 16) * 256LL > 0x3fffffffLL)
    return fail(-4, "d2d_stream_explored: grid too large for 32-bit indices inside one env");
  if (B == 0) return 0;
  if (!st || !st->dmap || !cells) return fail(-1, "d2d_stream_explored: a pointer is NULL");
  hipLaunchKernelGGL(stream_explored_kernel, dim3((unsigned)B), dim3(WAVE), 0, (hipStream_t)stream, *st, W, H, grid_tile, cells);
  return launched();
}

}  // extern "C"
