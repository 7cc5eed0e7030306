// d2d_render.hip — the renderer on the device (gfx950): the kernels + the C entry points of include/d2d_render.h and
// include/d2d_render_hooks.h.  Its own library (libd2d_render.so): it shares no kernel with the step, the closed loop, the planners
// or the observation channels, and it writes nothing of an env's state.
//
//   render_list    one wave per chosen slot, four a workgroup.  The wave reads the slot's trajectory length, decides whether the list
//                  fits, and its lanes then build item i = lane, lane + 64, ... (d2d_render_make: every item is a function of its
//                  index) and the item's pixel box.  count and status by lane 0.
//   render_bbox    the hook's first launch: one lane per item of a caller-made list, the pixel box.
//   render_frame   one workgroup of 256 lanes per (chosen slot, tile of 128 x 32 frame pixels); lane t owns the run of 16
//                  consecutive pixels [16 (t % 8), +16) of row t / 8: 48 bytes, three 16-byte stores where the run is whole and its
//                  address is a multiple of 16, single bytes at a ragged edge.
//                  cells   the run starts as the cell layer: one byte of the map per cell change, one division pair per run.
//                  cull    128 items a pass: lane t < 128 tests item c0 + t's 8-byte box against the tile's; the two waves' ballots
//                          compact the hits in list order into LDS (indices and boxes), then all lanes copy the kept records
//                          (176 bytes each) into LDS.
//                  paint   every lane walks the kept items in order -- the box against its run first, then d2d_render_covers per
//                          pixel -- over the 16 colours it holds in registers.  A list longer than a pass is more passes over the
//                          same registers: order is kept, nothing is dropped.
//   capture_select, render_list<true>, render_frame<true>   include/d2d_capture.h: one wave picks the finished slots a stream's harvest
//                  is about to record and gives each a frame of a gallery; the list and frame kernels under SEL skip the entries
//                  that name no slot, and a frame workgroup paints the frame its entry was given.  <false> is the text of before.
//
// Arithmetic is fp64 in the order include/d2d_render.h states, compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#define D2D_RENDER_QUAL __device__ __forceinline__
#define D2D_SINCOS_QUAL __device__ __forceinline__
#define D2D_SINCOS_TBL_QUAL __device__ const
#include "d2d_render.h"
#include "d2d_capture.h"

#define WAVE 64
#define LIST_WAVES 4
#define FRAME_LANES 256

namespace {

thread_local char g_err[256] = "";

int fail(int rc, const char *msg) {
  snprintf(g_err, sizeof g_err, "%s", msg);
  return rc;
}

// SEL (include/d2d_capture.h): an entry whose slot number is -1 is skipped -- the same text otherwise
template <bool SEL>
__global__ __launch_bounds__(LIST_WAVES *WAVE) void render_list_kernel(const d2d_cfg c, const double *__restrict__ drone,
                                                                      const double *__restrict__ agents,
                                                                      const uint8_t *__restrict__ active,
                                                                      const double *__restrict__ target,
                                                                      const int32_t *__restrict__ counters, const d2d_render_call r) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long k = (long long)blockIdx.x * LIST_WAVES + wv;
  if (k >= r.S) return;
  const int e = r.slots[k];
  if (SEL && e == -1) {  // no slot was chosen for this entry
    if (lane == 0) {
      r.count[k] = 0;
      r.status[k] = D2D_RENDER_SKIPPED;
    }
    return;
  }
  if (e < 0 || e >= c.B) {  // nothing of such a slot is read
    if (lane == 0) {
      r.count[k] = 0;
      r.status[k] = D2D_RENDER_BAD_SLOT;
    }
    return;
  }
  const int N = c.N;
  d2d_render_src s;
  s.drone = drone + (size_t)e * D2D_DF;
  s.agents = agents + (size_t)e * D2D_AF * N;
  s.active = active + (size_t)e * N;
  s.vel = r.agent_vel ? r.agent_vel + (size_t)e * 2 * N : nullptr;
  s.target = target + (size_t)e * 2;
  s.pillars = r.pillars + (size_t)e * r.P * 3;  // (never read with P == 0)
  s.star = r.star;
  s.N = N; s.P = r.P; s.n_seeded = r.n_seeded;
  s.steps = counters[(size_t)e * D2D_CF + D2D_C_STEPS];
  s.R = c.depth; s.range = r.view_range; s.drone_radius = c.drone_radius;
  s.traj = nullptr; s.traj_stride = 0; s.traj_len = 0;
  if (r.traj) {  // the caller's positions, 0 .. K of them
    int len = r.traj_len[k];
    len = len < 0 ? 0 : len > r.K ? r.K : len;
    s.traj = r.traj + (size_t)k * r.K * 2; s.traj_stride = 2; s.traj_len = len;
  } else if (r.plan_traj) {  // the device planner's: positions [head, stored) of its waypoints, both inside [0, plan_cap]
    int head = r.plan_hdr[(size_t)e * 2], stored = r.plan_hdr[(size_t)e * 2 + 1];
    stored = stored < 0 ? 0 : stored > r.plan_cap ? r.plan_cap : stored;
    head = head < 0 ? 0 : head > stored ? stored : head;
    s.traj = r.plan_traj + ((size_t)e * r.plan_cap + head) * 4; s.traj_stride = 4; s.traj_len = stored - head;
  }
  const int total = d2d_render_total(&s);
  if (total > r.cap) {
    if (lane == 0) {
      r.count[k] = 0;
      r.status[k] = D2D_RENDER_OVERFLOW;
    }
    return;
  }
  d2d_render_item *out = r.items + (size_t)k * r.cap;
  int16_t *box = r.bbox + (size_t)k * r.cap * 4;
  const int W_px = (int)c.W_px, H_px = (int)c.H_px;
  for (int i = lane; i < total; i += WAVE) {  // i < total <= cap: inside the slot's rows
    d2d_render_item it;
    d2d_render_make(&s, i, &it);
    out[i] = it;
    int16_t b[4];
    d2d_render_bbox(&it, W_px, H_px, b);
    *(short4 *)(box + 4 * i) = make_short4(b[0], b[1], b[2], b[3]);
  }
  if (lane == 0) {
    r.count[k] = total;
    r.status[k] = D2D_RENDER_OK;
  }
}

__global__ __launch_bounds__(256) void render_bbox_kernel(const d2d_render_item *__restrict__ items, const int32_t *__restrict__ count,
                                                          int16_t *__restrict__ bbox, const long long S, const int cap,
                                                          const int W_px, const int H_px) {
  const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
  if (a >= S * cap) return;
  const long long k = a / cap;
  const int i = (int)(a - k * cap);
  int16_t b[4] = {1, 1, 0, 0};
  if (i < count[k]) d2d_render_bbox(items + a, W_px, H_px, b);
  *(short4 *)(bbox + 4 * a) = make_short4(b[0], b[1], b[2], b[3]);
}

struct frame_args {
  const d2d_render_item *items;  // [S][cap]
  const int16_t *bbox;           // [S][cap][4]
  const int32_t *count;          // [S]
  const int32_t *slots;          // [S] or NULL: the grid of list k is grid k
  const uint8_t *grids;          // [B][grid_bytes]
  uint8_t *frame;                // [S][Hf][Wf][3]
  size_t grid_bytes;
  int B, cap, W, H, tile, scale, d, Wf, Hf, tiles_x, tiles_y;
};

// SEL (include/d2d_capture.h): list k paints frame dst[k]; a workgroup whose entry names no slot, or no frame of the gallery, is gone
// before any LDS use or barrier -- the slot number and dst[k] are the workgroup's, so no barrier is divergent
struct frame_sel {
  const int32_t *dst;  // [S]
  long long capacity;
};

template <bool SEL>
__global__ __launch_bounds__(FRAME_LANES) void render_frame_kernel(const frame_args a, const frame_sel sel) {
  __shared__ __attribute__((aligned(16))) double krec[D2D_RENDER_LDS_ITEMS * D2D_RENDER_ITEM_F64];
  __shared__ __attribute__((aligned(8))) int16_t kbox[D2D_RENDER_LDS_ITEMS * 4];
  __shared__ int kidx[D2D_RENDER_LDS_ITEMS];
  __shared__ int wcnt[2];

  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  const int per = a.tiles_x * a.tiles_y;
  const int k = blockIdx.x / per, tile = blockIdx.x - k * per;
  long long kf = k;  // the frame this workgroup paints
  if (SEL) {
    if (a.slots[k] == -1) return;
    kf = sel.dst[k];
    if (kf < 0 || kf >= sel.capacity) return;
  }
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int tu = tx * D2D_RENDER_TILE_W, tv = ty * D2D_RENDER_TILE_H;
  const int u0 = tu + (t & 7) * D2D_RENDER_RUN, v = tv + (t >> 3);
  const int d = a.d;
  int n = a.Wf - u0;
  n = n > D2D_RENDER_RUN ? D2D_RENDER_RUN : n;
  const bool mine = v < a.Hf && n > 0;  // a lane outside the frame holds no pixel and stores nothing; it still joins the barriers
  const int x0 = u0 * d, y = v * d;

  int e = a.slots ? a.slots[k] : k;
  const bool slot_ok = e >= 0 && e < a.B;  // a slot outside the batch has an empty list (render_list) and reads no map: UNEXPLORED
  int count = slot_ok ? a.count[k] : 0;
  count = count < 0 ? 0 : count > a.cap ? a.cap : count;

  uint32_t px[D2D_RENDER_RUN];
#pragma unroll
  for (int p = 0; p < D2D_RENDER_RUN; ++p) px[p] = 0x00f0f0f0u;
  if (mine && slot_ok) d2d_render_run_cells(a.grids + (size_t)e * a.grid_bytes, a.W, a.H, a.tile, a.scale, x0, y, d, n, px);

  const d2d_render_item *items = a.items + (size_t)k * a.cap;
  const int16_t *bbox = a.bbox + (size_t)k * a.cap * 4;
  const int tx0 = tu * d, ty0 = tv * d, tx1 = (tu + D2D_RENDER_TILE_W - 1) * d, ty1 = (tv + D2D_RENDER_TILE_H - 1) * d;
  for (int c0 = 0; c0 < count; c0 += D2D_RENDER_LDS_ITEMS) {  // (count is the workgroup's: every lane takes every barrier)
    // ---- cull: waves 0 and 1, one item a lane; the ballots keep list order ----
    short4 b = make_short4(1, 1, 0, 0);
    bool hit = false;
    const int i = c0 + t;
    if (t < D2D_RENDER_LDS_ITEMS && i < count) {
      b = *(const short4 *)(bbox + 4 * i);
      const int16_t bb[4] = {b.x, b.y, b.z, b.w};
      hit = d2d_render_box_hits(bb, tx0, ty0, tx1, ty1);
    }
    const unsigned long long m = __ballot(hit);
    if (wv < 2 && lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    const int nk = wcnt[0] + wcnt[1];
    if (hit) {
      const int q = (wv ? wcnt[0] : 0) + __popcll(m & ((1ull << lane) - 1ull));  // q < nk <= 128
      kidx[q] = i;
      *(short4 *)(kbox + 4 * q) = b;
    }
    __syncthreads();
    const double *src = (const double *)items;
    for (int q = t; q < nk * D2D_RENDER_ITEM_F64; q += FRAME_LANES) {
      const int rec = q / D2D_RENDER_ITEM_F64, f = q - rec * D2D_RENDER_ITEM_F64;
      krec[q] = src[(size_t)kidx[rec] * D2D_RENDER_ITEM_F64 + f];  // kidx < count <= cap
    }
    __syncthreads();
    // ---- paint ----
    if (mine) d2d_render_run_items((const d2d_render_item *)krec, kbox, nk, x0, y, d, n, px);
    __syncthreads();  // the next pass overwrites the list
  }
  if (!mine) return;

  // ---- store: 48 bytes whole, or the ragged edge byte by byte ----
  uint8_t *out = a.frame + (((size_t)kf * a.Hf + v) * a.Wf + u0) * 3;
  if (n == D2D_RENDER_RUN && ((uintptr_t)out & 15) == 0) {
    uint32_t w[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t p0 = px[4 * g], p1 = px[4 * g + 1], p2 = px[4 * g + 2], p3 = px[4 * g + 3];
      w[3 * g] = p0 | (p1 << 24);
      w[3 * g + 1] = (p1 >> 8) | (p2 << 16);
      w[3 * g + 2] = (p2 >> 16) | (p3 << 8);
    }
    uint4 *o = (uint4 *)out;
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
  } else {
#pragma unroll
    for (int p = 0; p < D2D_RENDER_RUN; ++p)
      if (p < n) {
        out[3 * p] = (uint8_t)px[p];
        out[3 * p + 1] = (uint8_t)(px[p] >> 8);
        out[3 * p + 2] = (uint8_t)(px[p] >> 16);
      }
  }
}

// One wave strides over the slots, 64 a pass.  The rank of a match is the carry of the passes before plus the pop-count of the
// ballot's bits below the lane: slot order, no atomics.  The accepted ranks are a prefix (r < S and r < room), so the -1 padding
// starts at their number.  Indices: r < S into sel_slot / sel_dst, taken + r < capacity into meta / pose, e < B into the state.
__global__ __launch_bounds__(WAVE) void capture_select_kernel(const int B, const uint8_t *__restrict__ flags,
                                                             const int32_t *__restrict__ counters, const double *__restrict__ drone,
                                                             const int32_t *__restrict__ slot_episode, const uint32_t kinds, const int S,
                                                             const long long capacity, int32_t *__restrict__ sel_slot,
                                                             int32_t *__restrict__ sel_dst, int32_t *__restrict__ meta,
                                                             double *__restrict__ pose, long long *counts) {
  const int lane = threadIdx.x;
  const long long taken = counts[0], dropped = counts[1], matched = counts[2];
  const long long room = d2d_capture_room(taken, capacity);
  long long carry = 0;
  for (int base = 0; base < B; base += WAVE) {
    const int e = base + lane;
    bool m = false;
    int kind = 0, ep = 0, steps = 0;
    if (e < B) {
      const uint8_t *f = flags + (size_t)e * 4;
      const int32_t *c = counters + (size_t)e * D2D_CF;
      ep = slot_episode ? slot_episode[e] : e;
      steps = c[D2D_C_STEPS];
      kind = d2d_capture_kind(f[D2D_F_COLLISION], f[D2D_F_DEADLOCK], f[D2D_F_FREEZING], c[D2D_C_SM]);
      m = d2d_capture_matches(f[D2D_F_DONE], ep, steps, kind, kinds);
    }
    const unsigned long long ballot = __ballot(m);
    const long long r = carry + __popcll(ballot & ((1ull << lane) - 1ull));
    if (m && r < S && r < room) {
      const long long row = taken + r;
      sel_slot[r] = e;
      sel_dst[r] = (int32_t)row;
      int32_t *mt = meta + row * D2D_CAPTURE_META_F;
      mt[D2D_CAPTURE_M_EPISODE] = ep;
      mt[D2D_CAPTURE_M_KIND] = kind;
      mt[D2D_CAPTURE_M_STEPS] = steps;
      mt[D2D_CAPTURE_M_SLOT] = e;
      const double *d = drone + (size_t)e * D2D_DF;
      pose[row * 3] = d[D2D_D_X];
      pose[row * 3 + 1] = d[D2D_D_Y];
      pose[row * 3 + 2] = d[D2D_D_YAW];
    }
    carry += __popcll(ballot);
  }
  long long accepted = carry < S ? carry : S;
  accepted = accepted < room ? accepted : room;
  for (long long i = accepted + lane; i < S; i += WAVE) sel_slot[i] = sel_dst[i] = -1;
  if (lane == 0) {  // every lane read counts before any write
    counts[0] = taken + accepted;
    counts[1] = dropped + (carry - accepted);
    counts[2] = matched + carry;
  }
}

int whole(double v, int *out) {
  if (!(v >= 1.0 && v <= 2147483647.0) || v != (double)(int)v) return 0;
  *out = (int)v;
  return 1;
}

int after_launch(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  snprintf(g_err, sizeof g_err, "%s: launch failed: %s", who, hipGetErrorString(err));
  return -3;
}

template <bool SEL = false>
int run_frame(frame_args a, long long S, int W_px, int H_px, void *stream, const char *who, frame_sel sel = frame_sel{nullptr, 0}) {
  a.Wf = (W_px + a.d - 1) / a.d;
  a.Hf = (H_px + a.d - 1) / a.d;
  a.tiles_x = (a.Wf + D2D_RENDER_TILE_W - 1) / D2D_RENDER_TILE_W;
  a.tiles_y = (a.Hf + D2D_RENDER_TILE_H - 1) / D2D_RENDER_TILE_H;
  hipLaunchKernelGGL(render_frame_kernel<SEL>, dim3((unsigned)(S * a.tiles_x * a.tiles_y)), dim3(FRAME_LANES), 0, (hipStream_t)stream, a,
                     sel);
  return after_launch(who);
}

}  // namespace

extern "C" {

int d2d_render_version(void) { return D2D_RENDER_VERSION; }
const char *d2d_render_last_error(void) { return g_err; }

static int check_call(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, const char *who, int *W_px, int *H_px, int *scale) {
  static thread_local char msg[200];
  const char *why = "";
  int rc = 0;
  if (!c || !s || !r) rc = -1, why = "cfg, state or call is NULL";
  else if (c->abi_version != D2D_ABI_VERSION) rc = -2, why = "the cfg has another D2D_ABI_VERSION";
  else if (c->B < 0 || c->N < 0 || r->S < 0 || r->P < 0 || r->K < 0 || r->plan_cap < 0 || r->cap < 1) rc = -1, why = "B, N, S, P, K, plan_cap >= 0, cap >= 1";
  else if (r->S == 0) return 0;
  else if (!r->slots || !r->items || !r->bbox || !r->count || !r->status) rc = -1, why = "slots, items, bbox, count or status is NULL";
  else if (!s->drone || !s->target || !s->counters || !s->dmap) rc = -1, why = "drone, target, counters or dmap is NULL";
  else if (c->N > 0 && (!s->agents || !s->active)) rc = -1, why = "agents or active is NULL with N > 0";
  else if (r->P > 0 && !r->pillars) rc = -1, why = "pillars is NULL with P > 0";
  else if (r->traj && !r->traj_len) rc = -1, why = "traj without traj_len";
  else if (r->plan_traj && !r->plan_hdr) rc = -1, why = "plan_traj without plan_hdr";
  else if (!whole(c->W_px, W_px) || !whole(c->H_px, H_px) || !whole(c->scale, scale)) rc = -4, why = "scale, W_px and H_px are whole numbers >= 1";
  else rc = d2d_render_check_geometry(r->S, r->cap, c->W, c->H, *W_px, *H_px, *scale, r->downsample, &why);
  if (rc) {
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return fail(rc, msg);
  }
  return 0;
}

static int run_list(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, void *stream, const char *who, bool sel) {
  int W_px, H_px, scale;
  const int rc = check_call(c, s, r, who, &W_px, &H_px, &scale);
  if (rc || r->S == 0) return rc;
  hipLaunchKernelGGL(sel ? render_list_kernel<true> : render_list_kernel<false>, dim3((unsigned)((r->S + LIST_WAVES - 1) / LIST_WAVES)), dim3(LIST_WAVES * WAVE), 0,
                     (hipStream_t)stream, *c, (const double *)s->drone, (const double *)s->agents, (const uint8_t *)s->active,
                     (const double *)s->target, (const int32_t *)s->counters, *r);
  return after_launch(who);
}

int d2d_render_list(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, void *stream) {
  return run_list(c, s, r, stream, "d2d_render_list", false);
}

int d2d_render_list_sel(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, void *stream) {
  return run_list(c, s, r, stream, "d2d_render_list_sel", true);
}

int d2d_render_frame(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, void *stream) {
  int W_px, H_px, scale;
  const int rc = check_call(c, s, r, "d2d_render_frame", &W_px, &H_px, &scale);
  if (rc || r->S == 0) return rc;
  if (!r->frame) return fail(-1, "d2d_render_frame: frame is NULL");
  if (c->grid_tile != 0 && c->grid_tile != 16) return fail(-1, "d2d_render_frame: grid_tile is 0 or 16");
  frame_args a = {r->items, r->bbox, r->count, r->slots, (const uint8_t *)s->dmap, r->frame, D2D_GRID_BYTES(c),
                  c->B, r->cap, c->W, c->H, c->grid_tile, scale, r->downsample, 0, 0, 0, 0};
  return run_frame(a, r->S, W_px, H_px, stream, "d2d_render_frame");
}

int d2d_render_frame_sel(const d2d_cfg *c, const d2d_state *s, const d2d_render_call *r, const int32_t *dst, int64_t capacity,
                         void *stream) {
  int W_px, H_px, scale;
  const int rc = check_call(c, s, r, "d2d_render_frame_sel", &W_px, &H_px, &scale);
  if (rc) return rc;
  if (capacity < 0 || capacity > 0x7fffffffLL) return fail(-1, "d2d_render_frame_sel: 0 <= capacity < 2^31");
  if (r->S == 0 || capacity == 0) return 0;
  if (!r->frame || !dst) return fail(-1, "d2d_render_frame_sel: frame or dst is NULL");
  if (c->grid_tile != 0 && c->grid_tile != 16) return fail(-1, "d2d_render_frame_sel: grid_tile is 0 or 16");
  frame_args a = {r->items, r->bbox, r->count, r->slots, (const uint8_t *)s->dmap, r->frame, D2D_GRID_BYTES(c),
                  c->B, r->cap, c->W, c->H, c->grid_tile, scale, r->downsample, 0, 0, 0, 0};
  return run_frame<true>(a, r->S, W_px, H_px, stream, "d2d_render_frame_sel", frame_sel{dst, (long long)capacity});
}

int d2d_capture_select(const d2d_cfg *c, const d2d_state *s, const int32_t *slot_episode, uint32_t kinds, int32_t S, int64_t capacity,
                       int32_t *sel_slot, int32_t *sel_dst, int32_t *meta, double *pose, int64_t *counts, void *stream) {
  if (!c || !s) return fail(-1, "d2d_capture_select: cfg or state is NULL");
  if (c->abi_version != D2D_ABI_VERSION) return fail(-2, "d2d_capture_select: the cfg has another D2D_ABI_VERSION");
  if (c->B < 0 || S < 0 || capacity < 0 || capacity > 0x7fffffffLL) return fail(-1, "d2d_capture_select: B, S >= 0, 0 <= capacity < 2^31");
  if (kinds >> D2D_CAPTURE_KINDS) return fail(-1, "d2d_capture_select: kinds has a bit beyond D2D_CAPTURE_KINDS");
  if (!counts) return fail(-1, "d2d_capture_select: counts is NULL");
  if (S > 0 && (!sel_slot || !sel_dst)) return fail(-1, "d2d_capture_select: sel_slot or sel_dst is NULL");
  if (capacity > 0 && (!meta || !pose)) return fail(-1, "d2d_capture_select: meta or pose is NULL");
  if (c->B > 0 && (!s->flags || !s->counters || !s->drone)) return fail(-1, "d2d_capture_select: flags, counters or drone is NULL");
  if (c->B == 0 && S == 0) return 0;
  hipLaunchKernelGGL(capture_select_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, (int)c->B, (const uint8_t *)s->flags,
                     (const int32_t *)s->counters, (const double *)s->drone, slot_episode, kinds, (int)S, (long long)capacity, sel_slot,
                     sel_dst, meta, pose, (long long *)counts);
  return after_launch("d2d_capture_select");
}

int d2d_render_raster(const d2d_render_raster_call *r, void *stream) {
  if (!r) return fail(-1, "d2d_render_raster: call is NULL");
  const char *why;
  const int rc = d2d_render_check_geometry(r->S, r->cap, r->W, r->H, r->W_px, r->H_px, r->scale, r->downsample, &why);
  if (rc) return fail(rc, why);
  if (r->S == 0) return 0;
  if (!r->items || !r->count || !r->cells || !r->bbox || !r->frame) return fail(-1, "d2d_render_raster: a buffer is NULL");
  const long long total = (long long)r->S * r->cap;
  hipLaunchKernelGGL(render_bbox_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r->items, r->count,
                     r->bbox, (long long)r->S, r->cap, r->W_px, r->H_px);
  const int rc2 = after_launch("d2d_render_raster");
  if (rc2) return rc2;
  frame_args a = {r->items, r->bbox, r->count, nullptr, r->cells, r->frame, (size_t)r->W * (size_t)r->H,
                  r->S, r->cap, r->W, r->H, 0, r->scale, r->downsample, 0, 0, 0, 0};
  return run_frame(a, r->S, r->W_px, r->H_px, stream, "d2d_render_raster");
}

}  // extern "C"
