// d2d_worlds.hip — the seeded worlds of a batch, built on the device (gfx950): kernels + the C entry points of
// include/d2d_worlds.h.  Its own library (libd2d_worlds.so): it shares no kernel with the step or the closed loop.
//
// Mapping: one wave per env, one workgroup per wave.  The wave keeps in LDS the Python stream's key behind a carry of
// D2D_W_CARRY words, the pillars and the accepted agents (x, y, r) -- never a grid: the grids are written straight to
// global memory, cell by cell of their byte range, whatever their size.
//
//   seeding     init_genrand + init_by_array (1 870 dependent integer steps) and numpy's init_genrand (623) run on lane 0 over
//               LDS; the first regeneration of either key is wave-parallel (64 words per pass, in place).
//   pillars     a handful of randint draws with redraws: uniform over the wave, every lane reads the same words.
//   agents      lane j evaluates attempt j of a pass (six words from the stream's position on, whatever the attempts before it
//               decide) against the accepted list, the pillars and the start; the first free lane (ballot, find-first) is
//               accepted, the lanes behind it test the newcomer too, and so on through the pass.  The stream ends behind the
//               attempt that completes the list.  An attempt never straddles a regeneration: when fewer than six words are
//               left they move into the carry in front of the key before it is regenerated, so any position works (pillars
//               leave the stream anywhere).
//   records     lane = agent: pow(r, 2.0) (d2d_pow2), the floor divisions, the static map's velocities (d2d_sincos) from the
//               numpy key; then the wave covers each agent's block of cells.
//   grids       lane = four consecutive bytes of the env's grid storage, row-major or tiled; the agents' DYNAMIC cells follow
//               behind a workgroup barrier, and since they all write the same value their order does not matter.
//
// The episode stream (include/d2d_worlds_stream.h) lives here too: worlds_build_masked_kernel is the same body (d2d_worlds_build.inc,
// shared as text) behind a refill byte, stream_harvest_kernel (one wave per slot) records a finished slot's row, stream_assign_kernel
// (one workgroup) hands the finished slots their next map ids by a ballot scan -- consecutive ones, or with include/d2d_worlds_table.h
// the rows of an episode table --, stream_clear_kernel zeroes a refilled slot's rows of a buffer.  The turn of a stream the caller
// steps itself (include/d2d_worlds_turn.h) is the tail of this file, d2d_worlds_turn.inc: stream_restore_kernel puts back a refilled
// slot's ranges outside the world in one launch, stream_explored_kernel counts every slot's discovered cells with the harvest's own
// text (d2d_stream_count.inc).
//
// Every loop is bounded by d2d_world_spec.max_attempts or by a size of the spec.  Arithmetic is fp64 in the reference's own
// operation order, compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_WORLDS_QUAL __device__ __forceinline__
#define D2D_RNG_QUAL __device__ __forceinline__
#define D2D_LOG_QUAL __device__ __forceinline__
#define D2D_LOG_TBL_QUAL __device__ const
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#define D2D_POW2_QUAL __device__ __forceinline__
#define D2D_POW2_TBL_QUAL __device__ const
#include "d2d_worlds.h"
#include "../../../include/d2d_worlds_stream.h"
#include "../../../include/d2d_worlds_table.h"
#include "d2d_restore.h"

#define WAVE 64

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

// The next key, in place: 64 words per pass in ascending order, the order the sequential algorithm writes them in.  Word i reads
// words i + 1 (old; the last one reads the new word 0) and i + 397 mod 624 (old below i = 227, new from there on): never a word of
// its own pass except i + 1, which its neighbour replaces -- so a pass reads, then writes.
__device__ __forceinline__ void wave_regen(uint32_t *key, int lane) {
  for (int i0 = 0; i0 < D2D_RNG_KEY; i0 += WAVE) {
    const int i = i0 + lane;
    uint32_t v = 0;
    if (i < D2D_RNG_KEY) {
      const int i1 = i + 1 == D2D_RNG_KEY ? 0 : i + 1;
      const int im = i + D2D_RNG_M >= D2D_RNG_KEY ? i + D2D_RNG_M - D2D_RNG_KEY : i + D2D_RNG_M;
      v = d2d_rng_twist(key[i], key[i1], key[im]);
    }
    __syncthreads();
    if (i < D2D_RNG_KEY) key[i] = v;
    __syncthreads();
  }
}

// Make `need` (<= D2D_W_CARRY) words readable at buf[p ..]: when the key holds fewer, what it still holds moves into the carry in
// front of it and the key is regenerated behind.  p is an index into buf, D2D_W_BUF = the end of the key.
__device__ __forceinline__ void stream_ensure(uint32_t *buf, int &p, int need, int lane) {
  const int avail = D2D_W_BUF - p;
  if (avail >= need) return;
  uint32_t t = 0;
  if (lane < avail) t = buf[p + lane];
  __syncthreads();
  if (lane < avail) buf[D2D_W_CARRY - avail + lane] = t;
  wave_regen(buf + D2D_W_CARRY, lane);
  p = D2D_W_CARRY - avail;
}

// bytes [0, G) behind p from value(byte index): whole aligned words where the address allows, single bytes at the two ends
template <typename F>
__device__ __forceinline__ void fill_bytes(uint8_t *p, int G, int lane, F &&value) {
  int head = (int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u);
  if (head > G) head = G;
  if (lane < head) p[lane] = value(lane);
  const int nw = (G - head) >> 2;
  uint32_t *w = (uint32_t *)(p + head);
  for (int q = lane; q < nw; q += WAVE) {
    const int b = head + 4 * q;
    w[q] = (uint32_t)value(b) | ((uint32_t)value(b + 1) << 8) | ((uint32_t)value(b + 2) << 16) | ((uint32_t)value(b + 3) << 24);
  }
  const int t0 = head + 4 * nw;
  if (t0 + lane < G) p[t0 + lane] = value(t0 + lane);
}

__device__ __forceinline__ double shfl_f64(double v, int src) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = __shfl((unsigned)b, src, WAVE), hi = __shfl((unsigned)(b >> 32), src, WAVE);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(WAVE) void worlds_build_kernel(const d2d_world_spec s, const d2d_state st) {
#include "d2d_worlds_build.inc"   // the body, shared as text with worlds_build_masked_kernel
}

// d2d_worlds_build for the slots of a stream that were just handed a new episode (include/d2d_worlds_stream.h): one wave per slot,
// and a wave whose refill byte is 0 is gone before it reads anything else.  The flags of a rebuilt slot are written here, as one
// word: a slot that hit max_attempts is done from this launch on, so no later launch steps it.
__global__ __launch_bounds__(WAVE) void worlds_build_masked_kernel(const d2d_world_spec s, const d2d_state st, const uint8_t *refill) {
  if (!refill[blockIdx.x]) return;
#include "d2d_worlds_build.inc"
  if (st.flags && lane < 4) st.flags[(size_t)e * 4 + lane] = (uint8_t)((!ok && lane == D2D_STREAM_F_DONE) ? 1 : 0);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

// non-zero bytes among the low `n` (0 .. 4) bytes of w
__device__ __forceinline__ int nonzero_bytes(uint32_t w, int n) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c += (k < n && ((w >> (8 * k)) & 0xffu)) ? 1 : 0;
  return c;
}

// One wave per slot: the record of a finished episode.  dmap's cells are counted a word at a time where the address allows.  Row-major:
// an env's grid starts anywhere (W * H need not be a multiple of 4), so single bytes at the two ends, as fill_bytes writes them.
// Tiled: an env's grid is whole tiles of 256 bytes, a word lies inside one row of one tile, and of its four cells those with j < H
// of a row i < W count -- the padding is skipped, whatever it holds.
__global__ __launch_bounds__(WAVE) void stream_harvest_kernel(const d2d_state st, const int32_t *slot_episode, int W, int H, int tile,
                                                             long long M, int32_t *rows) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (!st.flags[(size_t)e * 4 + D2D_STREAM_F_DONE]) return;
  const int ep = slot_episode[e];
  if (ep < 0 || (long long)ep >= M) return;
#include "d2d_stream_count.inc"   // cnt: the non-zero cells of the slot's dmap, shared as text with stream_explored_kernel
  if (lane < D2D_STREAM_ROW_F) {
    const int32_t *c = st.counters + (size_t)e * D2D_CF;
    const uint8_t *f = st.flags + (size_t)e * 4;
    const int32_t v = lane == D2D_STREAM_R_STEPS ? c[D2D_C_STEPS] : lane == D2D_STREAM_R_SM ? c[D2D_C_SM]
                    : lane == D2D_STREAM_R_BUF_N ? c[D2D_C_BUF_N] : lane == D2D_STREAM_R_BUF_TS ? c[D2D_C_BUF_TS]
                    : lane == D2D_STREAM_R_DMAP ? cnt : (int32_t)f[lane - D2D_STREAM_R_FLAG0];
    rows[(size_t)ep * D2D_STREAM_ROW_F + lane] = v;
  }
}

// One workgroup strides over the slots.  The exclusive scan of "harvested" is a ballot inside a wave, the waves' totals through LDS
// inside a stride, and a carry from stride to stride: no atomics, so the assignment is a function of the flags alone.
// TABLE: episode k is row k of a table (include/d2d_worlds_table.h) and the slot that receives it copies the row -- its map id, its
// env_par and its env_tgt -- where the consecutive form writes map_id0 + k; the scan is the same text.
struct episode_table {
  const uint32_t *ep_map_id;   // [M]
  const double *ep_par;        // [M][D2D_WORLDS_ENV_F]
  const double *ep_tgt;        // [M][T][2]
  double *env_par, *env_tgt;   // [B][..]: what d2d_worlds_build_masked reads
  int T;
};
#define ASSIGN_BLOCK 1024
template <bool TABLE>
__global__ __launch_bounds__(ASSIGN_BLOCK) void stream_assign_kernel(const uint8_t *flags, int B, long long M, uint32_t map_id0,
                                                                    int32_t *slot_episode, uint32_t *map_id, uint8_t *refill,
                                                                    long long *counts, const episode_table tb) {
  __shared__ int wave_total[ASSIGN_BLOCK / WAVE];
  const int tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
  const long long cursor = counts[0], finished = counts[1];
  long long carry = 0;
  for (int base = 0; base < B; base += ASSIGN_BLOCK) {
    const int e = base + tid;
    const bool h = e < B && flags[(size_t)e * 4 + D2D_STREAM_F_DONE] != 0 && slot_episode[e] >= 0;
    const unsigned long long m = __ballot(h);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wv] = __popcll(m);
    __syncthreads();
    int below = 0, total = 0;
    for (int k = 0; k < ASSIGN_BLOCK / WAVE; ++k) {
      const int t = wave_total[k];
      below += k < wv ? t : 0;
      total += t;
    }
    if (e < B) {
      if (h) {
        const long long k = cursor + carry + below + before;
        if (k < M) {
          slot_episode[e] = (int32_t)k;
          if (TABLE) {
            map_id[e] = tb.ep_map_id[k];
            for (int i = 0; i < D2D_WORLDS_ENV_F; ++i) tb.env_par[(size_t)e * D2D_WORLDS_ENV_F + i] = tb.ep_par[(size_t)k * D2D_WORLDS_ENV_F + i];
            for (int i = 0; i < 2 * tb.T; ++i) tb.env_tgt[(size_t)e * 2 * tb.T + i] = tb.ep_tgt[(size_t)k * 2 * tb.T + i];
          } else {
            map_id[e] = map_id0 + (uint32_t)k;
          }
          refill[e] = 1;
        } else {
          slot_episode[e] = -1;
          refill[e] = 0;
        }
      } else {
        refill[e] = 0;
      }
    }
    carry += total;
    __syncthreads();      // wave_total is rewritten by the next stride
  }
  if (tid == 0) {         // every thread read counts before the first barrier; B == 0 launches nothing
    counts[0] = cursor + carry < M ? cursor + carry : M;
    counts[1] = finished + carry;
  }
}

// Zero the rows of the refilled slots of one per-slot buffer ([B][words] of 32 bits): one workgroup per slot, gone after reading its
// refill byte where that is 0.  For the per-slot state no masked reset covers (the trajectory storage, the search scratch, the
// scratch half of the RVO velocities): cost follows the slots rebuilt, not the batch.
#define CLEAR_BLOCK 256
__global__ __launch_bounds__(CLEAR_BLOCK) void stream_clear_kernel(uint32_t *base, long long words, const uint8_t *refill) {
  if (!refill[blockIdx.x]) return;
  uint32_t *row = base + (size_t)blockIdx.x * (size_t)words;
  for (long long i = threadIdx.x; i < words; i += CLEAR_BLOCK) row[i] = 0u;
}

size_t lds_bytes(const d2d_world_spec *s) {
  return sizeof(double) * D2D_W_ACC_F * (size_t)s->n_rand + sizeof(uint32_t) * D2D_W_BUF + sizeof(int32_t) * 3 * (size_t)s->P;
}

int check_spec(const d2d_world_spec *s) {
  if (!s) return fail(-1, "d2d_worlds: spec is NULL");
  if (s->version != D2D_WORLDS_VERSION) return fail(-2, "d2d_worlds: spec.version != D2D_WORLDS_VERSION");
  if (s->B < 0 || s->n_rand < 0 || s->n_cells < 0 || s->P < 0 || s->N != s->n_rand + s->n_cells || s->T < 1)
    return fail(-1, "d2d_worlds: B, n_rand, n_cells, P >= 0, N = n_rand + n_cells, T >= 1");
  if (s->scale < 1 || s->W_px < 1 || s->H_px < 1 || s->W != s->W_px / s->scale || s->H != s->H_px / s->scale || s->W < 1 || s->H < 1)
    return fail(-1, "d2d_worlds: W = W_px / scale, H = H_px / scale, all positive");
  if (s->grid_tile != 0 && s->grid_tile != 16) return fail(-1, "d2d_worlds: grid_tile is 0 or 16");
  if (s->max_attempts < 1) return fail(-1, "d2d_worlds: max_attempts >= 1");
  if (s->P > 0 && (s->W_px < 100 || s->H_px < 100)) return fail(-1, "d2d_worlds: pillars need a map of at least 100 x 100 px");
  if (((long long)(s->W + 15) / 16) * ((s->H + 15) / 16) * 256LL > 0x3fffffffLL || (long long)s->N * D2D_KF > 0x3fffffffLL)
    return fail(-4, "d2d_worlds: grid or agent list too large for 32-bit indices inside one env");
  if (lds_bytes(s) > 64u * 1024u) return fail(-4, "d2d_worlds: accepted list and pillars exceed 64 KB of LDS");
  return 0;
}

int check_arrays(const d2d_world_spec *spec, const d2d_state *st) {
  if (!spec->map_id || !spec->env_par || !spec->env_tgt || !spec->status || (spec->n_rand && !spec->unit) ||
      (spec->n_cells && !spec->cells) || (spec->N && !spec->tracker_radius) || (spec->P && !spec->obstacles))
    return fail(-1, "d2d_worlds: a spec array is NULL");
  if (!st->gt || !st->dmap || !st->drone || !st->target || !st->targets || !st->counters ||
      (spec->N && (!st->agents || !st->agent_unit || !st->dyn_prev || !st->active)))
    return fail(-1, "d2d_worlds: a world field of the state is NULL");
  return 0;
}

int launched() {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    snprintf(g_err, sizeof g_err, "d2d_worlds: launch failed: %s", hipGetErrorString(err));
    return -3;
  }
  return 0;
}

}  // namespace

extern "C" {

int d2d_worlds_version(void) { return D2D_WORLDS_VERSION; }
const char *d2d_worlds_last_error(void) { return g_err; }

int d2d_worlds_launch_shape(const d2d_world_spec *spec, int32_t out[2]) {
  if (const int rc = check_spec(spec)) return rc;
  if (!out) return fail(-1, "d2d_worlds: out is NULL");
  out[0] = 1;
  out[1] = (int32_t)lds_bytes(spec);
  return 0;
}

int d2d_worlds_build(const d2d_world_spec *spec, const d2d_state *st, void *stream) {
  if (const int rc = check_spec(spec)) return rc;
  if (!st) return fail(-1, "d2d_worlds: state is NULL");
  if (spec->B == 0) return 0;
  if (const int rc = check_arrays(spec, st)) return rc;
  hipLaunchKernelGGL(worlds_build_kernel, dim3((unsigned)spec->B), dim3(WAVE), lds_bytes(spec), (hipStream_t)stream, *spec, *st);
  return launched();
}

int d2d_worlds_build_masked(const d2d_world_spec *spec, const d2d_state *st, const uint8_t *refill, void *stream) {
  if (const int rc = check_spec(spec)) return rc;
  if (!st) return fail(-1, "d2d_worlds: state is NULL");
  if (spec->B == 0) return 0;
  if (!refill) return fail(-1, "d2d_worlds_build_masked: refill is NULL (d2d_worlds_build is the launch without a mask)");
  if (const int rc = check_arrays(spec, st)) return rc;
  hipLaunchKernelGGL(worlds_build_masked_kernel, dim3((unsigned)spec->B), dim3(WAVE), lds_bytes(spec), (hipStream_t)stream, *spec, *st,
                     refill);
  return launched();
}

int d2d_stream_harvest(const d2d_state *st, const int32_t *slot_episode, int32_t B, int32_t W, int32_t H, int32_t grid_tile, int64_t M,
                       int32_t *rows, void *stream) {
  if (B < 0 || W < 1 || H < 1 || M < 0 || M > D2D_STREAM_MAX_EPISODES) return fail(-1, "d2d_stream_harvest: B >= 0, W, H >= 1, 0 <= M <= D2D_STREAM_MAX_EPISODES");
  if (grid_tile != 0 && grid_tile != 16) return fail(-1, "d2d_stream_harvest: grid_tile is 0 or 16");
  if (((long long)(W + 15) / 16) * ((H + 15) / 16) * 256LL > 0x3fffffffLL)
    return fail(-4, "d2d_stream_harvest: grid too large for 32-bit indices inside one env");
  if (B == 0 || M == 0) return 0;
  if (!st || !st->flags || !st->counters || !st->dmap || !slot_episode || !rows) return fail(-1, "d2d_stream_harvest: a pointer is NULL");
  hipLaunchKernelGGL(stream_harvest_kernel, dim3((unsigned)B), dim3(WAVE), 0, (hipStream_t)stream, *st, slot_episode, W, H, grid_tile,
                     (long long)M, rows);
  return launched();
}

int d2d_stream_assign(const uint8_t *flags, int32_t B, int64_t M, uint32_t map_id0, int32_t *slot_episode, uint32_t *map_id,
                      uint8_t *refill, int64_t *counts, void *stream) {
  if (B < 0 || M < 0 || M > D2D_STREAM_MAX_EPISODES) return fail(-1, "d2d_stream_assign: B >= 0, 0 <= M <= D2D_STREAM_MAX_EPISODES");
  if ((unsigned long long)map_id0 + (unsigned long long)M > 0x100000000ULL) return fail(-1, "d2d_stream_assign: map_id0 + M > 2^32");
  if (B == 0) return 0;
  if (!flags || !slot_episode || !map_id || !refill || !counts) return fail(-1, "d2d_stream_assign: a pointer is NULL");
  hipLaunchKernelGGL(stream_assign_kernel<false>, dim3(1), dim3(ASSIGN_BLOCK), 0, (hipStream_t)stream, flags, B, (long long)M, map_id0,
                     slot_episode, map_id, refill, (long long *)counts, episode_table{});
  return launched();
}

int d2d_stream_assign_table(const uint8_t *flags, int32_t B, int64_t M, int32_t T, const uint32_t *ep_map_id, const double *ep_par,
                            const double *ep_tgt, int32_t *slot_episode, uint32_t *map_id, double *env_par, double *env_tgt,
                            uint8_t *refill, int64_t *counts, void *stream) {
  if (B < 0 || M < 0 || M > D2D_STREAM_MAX_EPISODES || T < 1)
    return fail(-1, "d2d_stream_assign_table: B >= 0, 0 <= M <= D2D_STREAM_MAX_EPISODES, T >= 1");
  if (B == 0) return 0;
  if (!flags || !slot_episode || !map_id || !env_par || !env_tgt || !refill || !counts)
    return fail(-1, "d2d_stream_assign_table: a pointer is NULL");
  if (M > 0 && (!ep_map_id || !ep_par || !ep_tgt)) return fail(-1, "d2d_stream_assign_table: a table pointer is NULL");
  const episode_table tb = {ep_map_id, ep_par, ep_tgt, env_par, env_tgt, (int)T};
  hipLaunchKernelGGL(stream_assign_kernel<true>, dim3(1), dim3(ASSIGN_BLOCK), 0, (hipStream_t)stream, flags, B, (long long)M, 0u,
                     slot_episode, map_id, refill, (long long *)counts, tb);
  return launched();
}

int d2d_stream_clear(void *base, int64_t bytes_per_slot, const uint8_t *refill, int32_t B, void *stream) {
  if (B < 0 || bytes_per_slot < 0 || (bytes_per_slot & 3) || ((uintptr_t)base & 3u))
    return fail(-1, "d2d_stream_clear: B >= 0, bytes_per_slot a multiple of 4 and >= 0, base aligned to 4 bytes");
  if (B == 0 || bytes_per_slot == 0) return 0;
  if (!base || !refill) return fail(-1, "d2d_stream_clear: a pointer is NULL");
  hipLaunchKernelGGL(stream_clear_kernel, dim3((unsigned)B), dim3(CLEAR_BLOCK), 0, (hipStream_t)stream, (uint32_t *)base,
                     (long long)(bytes_per_slot >> 2), refill);
  return launched();
}

}  // extern "C"

#include "d2d_worlds_turn.inc"   // d2d_stream_restore, d2d_stream_explored (include/d2d_worlds_turn.h)
