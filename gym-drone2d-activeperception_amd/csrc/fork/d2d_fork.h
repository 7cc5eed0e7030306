/*
 * d2d_fork.h — the scalar logic of d2d_fork_slots (include/d2d_fork.h): what a destination slot's status is, and what thread `tid`
 * of workgroup `part` of a slot copies for one item.  One text for the device kernel (d2d_fork.hip) and for the host build that
 * checks the range arithmetic and the byte ends under a sanitizer (tests/csrc/fork_host.c, fork_host_main.c): the thread index is a
 * parameter.
 *
 * A row of an item is bytes [0, n) behind d = dst + e * dst_stride, read from p = src + s * src_stride.  With the unit u = 16 where
 * d and p agree modulo 16, 4 where they agree modulo 4 only, 1 otherwise:
 *   head   the (u - d % u) % u bytes in front of the first aligned unit, at most n        (single bytes)
 *   units  nu = (n - head) / u whole units, aligned in the source and in the destination  (one access of u bytes each)
 *   tail   the (n - head) % u bytes behind them                                            (single bytes)
 * A row of more than D2D_FORK_SMALL_BYTES is cut into D2D_FORK_PARTS runs of ceil(nu / parts) units, run p for workgroup p, and
 * workgroup 0 copies the two ends; a smaller row belongs whole to workgroup (item index % parts).  Every byte of the row is written
 * by exactly one thread of one workgroup, and no other byte is read or written.  A thread's units are taken four at a time, the
 * four loads in front of the four stores: source and destination are never the same slot, so no load needs an earlier store.
 */
#ifndef D2D_FORK_IMPL_H
#define D2D_FORK_IMPL_H

#include <stdint.h>

#include "../../../include/d2d_fork.h"

#ifndef D2D_FORK_QUAL
#define D2D_FORK_QUAL static inline
#endif

#define D2D_FORK_BLOCK 64 /* one wave */

/* the device build names the address space of the rows (global memory: the accesses are global_, not flat_); the host has one */
#ifndef D2D_FORK_MEM
#define D2D_FORK_MEM
#endif

/* sixteen bytes at a 16-byte boundary: one access */
typedef struct __attribute__((aligned(16), may_alias)) d2d_fork_quad {
  uint32_t a, b, c, d;
} d2d_fork_quad;
typedef uint32_t __attribute__((may_alias)) d2d_fork_word;

/* status of destination slot e: D2D_FORK_LEFT / COPIED / REFUSED.  Reads src_of[e] and, in place, src_of[src_of[e]] */
D2D_FORK_QUAL int d2d_fork_decide(const int32_t *src_of, int64_t e, int32_t B_src, int in_place) {
  const int32_t s = src_of[e];
  if (s < 0) return D2D_FORK_LEFT;
  if (s >= B_src) return D2D_FORK_REFUSED;
  if (!in_place) return D2D_FORK_COPIED;
  if (s == e) return D2D_FORK_LEFT;
  const int32_t t = src_of[s]; /* s < B_src == B_dst */
  return (t < 0 || t == s) ? D2D_FORK_COPIED : D2D_FORK_REFUSED;
}

/* units [u0, u1) of d <- p for thread tid of nthreads, four in flight */
#define D2D_FORK_RUN(type, dp, pp, u0, u1)                                                    \
  do {                                                                                        \
    D2D_FORK_MEM type *dv_ = (D2D_FORK_MEM type *)(dp);                                       \
    const D2D_FORK_MEM type *pv_ = (const D2D_FORK_MEM type *)(pp);                           \
    const int64_t nt_ = nthreads;                                                             \
    int64_t q_ = (u0) + tid;                                                                  \
    for (; q_ + 3 * nt_ < (u1); q_ += 4 * nt_) {                                              \
      const type x0_ = pv_[q_], x1_ = pv_[q_ + nt_], x2_ = pv_[q_ + 2 * nt_], x3_ = pv_[q_ + 3 * nt_]; \
      dv_[q_] = x0_;                                                                          \
      dv_[q_ + nt_] = x1_;                                                                    \
      dv_[q_ + 2 * nt_] = x2_;                                                                \
      dv_[q_ + 3 * nt_] = x3_;                                                                \
    }                                                                                         \
    for (; q_ < (u1); q_ += nt_) dv_[q_] = pv_[q_];                                           \
  } while (0)

/* thread `tid` of `nthreads` of workgroup `part` of destination slot e <- source slot s, item number `index` */
D2D_FORK_QUAL void d2d_fork_copy_row(const d2d_fork_item *it, int index, int64_t e, int64_t s, int part, int tid, int nthreads) {
  const int64_t n = it->bytes;
  if (n <= 0) return;
  D2D_FORK_MEM uint8_t *d = (D2D_FORK_MEM uint8_t *)it->dst + e * it->dst_stride;
  const D2D_FORK_MEM uint8_t *p = (const D2D_FORK_MEM uint8_t *)it->src + s * it->src_stride;
  const unsigned diff = (unsigned)((uintptr_t)d - (uintptr_t)p);
  const int unit = (diff & 15u) == 0 ? 16 : ((diff & 3u) == 0 ? 4 : 1);
  int64_t head = (int64_t)(((unsigned)unit - (unsigned)((uintptr_t)d & (uintptr_t)(unit - 1))) & (unsigned)(unit - 1));
  if (head > n) head = n;
  const int64_t nu = (n - head) / unit, tail0 = head + nu * unit;
  int64_t u0, u1;
  int ends;
  if (n <= D2D_FORK_SMALL_BYTES) {
    ends = part == index % D2D_FORK_PARTS;
    u0 = 0;
    u1 = ends ? nu : 0;
  } else {
    const int64_t run = (nu + D2D_FORK_PARTS - 1) / D2D_FORK_PARTS;
    ends = part == 0;
    u0 = (int64_t)part * run < nu ? (int64_t)part * run : nu;
    u1 = u0 + run < nu ? u0 + run : nu;
  }
  if (ends) { /* at most fifteen bytes at either end */
    for (int64_t b = tid; b < head; b += nthreads) d[b] = p[b];
    for (int64_t b = tail0 + tid; b < n; b += nthreads) d[b] = p[b];
  }
  if (unit == 16) D2D_FORK_RUN(d2d_fork_quad, d + head, p + head, u0, u1);
  else if (unit == 4) D2D_FORK_RUN(d2d_fork_word, d + head, p + head, u0, u1);
  else D2D_FORK_RUN(uint8_t, d, p, u0, u1);
}

/* the argument checks of d2d_fork_slots: 0, or the error code with *why the message */
D2D_FORK_QUAL int d2d_fork_check(const d2d_fork_item *items, int32_t n_items, const int32_t *src_of, int32_t B_dst, int32_t B_src,
                                 int32_t in_place, const uint8_t *status, const char **why) {
  *why = "";
  if (B_dst < 0 || B_src < 0) return *why = "d2d_fork_slots: B_dst, B_src >= 0", -1;
  if (n_items < 0 || n_items > D2D_FORK_MAX_ITEMS) return *why = "d2d_fork_slots: 0 <= n_items <= D2D_FORK_MAX_ITEMS (64)", -1;
  if (in_place && B_src != B_dst) return *why = "d2d_fork_slots: in place the source is the destination, B_src == B_dst", -1;
  if ((long long)B_dst * D2D_FORK_PARTS > 0x7fffffffLL) return *why = "d2d_fork_slots: B_dst * D2D_FORK_PARTS workgroups exceed the grid", -4;
  if (B_dst == 0) return 0;
  if (!src_of || !status || (n_items && !items)) return *why = "d2d_fork_slots: a pointer is NULL", -1;
  if ((uintptr_t)items & 7u) return *why = "d2d_fork_slots: items aligned to 8 bytes", -1;
  if ((uintptr_t)src_of & 3u) return *why = "d2d_fork_slots: src_of aligned to 4 bytes", -1;
  return 0;
}

#endif /* D2D_FORK_IMPL_H */
