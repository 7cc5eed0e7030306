/*
 * d2d_restore.h — the scalar item logic of d2d_stream_restore (include/d2d_worlds_turn.h): what thread `tid` of workgroup `part` of
 * a slot writes for one item.  One text for the device kernel (d2d_worlds_turn.inc) and for the host build that checks the range
 * arithmetic and the byte ends under a sanitizer (tests/csrc/restore_host_main.c).
 *
 * A slot's range of an item is bytes [0, n) behind d = dst + e * dst_stride + dst_off:
 *   head   the (4 - d % 4) % 4 bytes in front of the first aligned word, at most n
 *   words  nw = (n - head) / 4 whole words; a run of zeroes is stored four words at a time between its 16-byte boundaries
 *   tail   the (n - head) % 4 bytes behind them
 * An item of more than D2D_RESTORE_SMALL_WORDS words is cut into D2D_RESTORE_PARTS runs of ceil(nw / parts) words, run p for
 * workgroup p, and workgroup 0 writes the two ends; a smaller item belongs whole to workgroup (item index % parts).  Every byte of
 * the range is written by exactly one thread of one workgroup, and no other byte is written.
 */
#ifndef D2D_RESTORE_IMPL_H
#define D2D_RESTORE_IMPL_H

#include <stdint.h>

#include "../../../include/d2d_worlds_turn.h"

#ifndef D2D_WORLDS_QUAL
#define D2D_WORLDS_QUAL static inline
#endif

#ifndef D2D_RESTORE_BLOCK
#define D2D_RESTORE_BLOCK 64 /* one wave: 8 waves a slot; four times the waves cost up to 3.5x with every slot set and gain nothing with one */
#endif
#define D2D_RESTORE_SMALL_WORDS 1024

/* four words at a 16-byte boundary: one store */
typedef struct __attribute__((aligned(16))) d2d_restore_quad {
  uint32_t a, b, c, d;
} d2d_restore_quad;

/* byte b of the source as a D2D_RESTORE_COPY reads it */
D2D_WORLDS_QUAL uint32_t d2d_restore_word(const uint8_t *s, int64_t b, int aligned) {
  if (aligned) return *(const uint32_t *)(s + b);
  return (uint32_t)s[b] | ((uint32_t)s[b + 1] << 8) | ((uint32_t)s[b + 2] << 16) | ((uint32_t)s[b + 3] << 24);
}

/* thread `tid` of `nthreads` of workgroup `part` of slot e, item number `index` */
D2D_WORLDS_QUAL void d2d_restore_apply(const d2d_restore_item *it, int index, int64_t e, int part, int tid, int nthreads) {
  const int64_t n = it->bytes;
  const int copy = it->kind == D2D_RESTORE_COPY;
  if (n <= 0 || (!copy && it->kind != D2D_RESTORE_ZERO)) return;
  uint8_t *d = (uint8_t *)it->dst + e * it->dst_stride + it->dst_off;
  const uint8_t *s = copy ? (const uint8_t *)it->src + e * it->src_stride + it->src_off : (const uint8_t *)0;
  int64_t head = (int64_t)((4u - (unsigned)((uintptr_t)d & 3u)) & 3u);
  if (head > n) head = n;
  const int64_t nw = (n - head) >> 2, tail0 = head + 4 * nw;
  int64_t w0, w1;
  int ends;
  if (nw <= D2D_RESTORE_SMALL_WORDS) {
    ends = part == index % D2D_RESTORE_PARTS;
    w0 = 0;
    w1 = ends ? nw : 0;
  } else {
    const int64_t run = (nw + D2D_RESTORE_PARTS - 1) / D2D_RESTORE_PARTS;
    ends = part == 0;
    w0 = (int64_t)part * run < nw ? (int64_t)part * run : nw;
    w1 = w0 + run < nw ? w0 + run : nw;
  }
  if (ends) {                      /* at most three bytes at either end */
    if (tid < head) d[tid] = copy ? s[tid] : (uint8_t)0;
    if (tail0 + tid < n) d[tail0 + tid] = copy ? s[tail0 + tid] : (uint8_t)0;
  }
  uint32_t *w = (uint32_t *)(d + head);
  if (copy) {
    const int aligned = ((uintptr_t)(s + head) & 3u) == 0;
    for (int64_t q = w0 + tid; q < w1; q += nthreads) w[q] = d2d_restore_word(s, head + 4 * q, aligned);
    return;
  }
  /* zeroes: the run's words up to the first 16-byte boundary, whole quads of words, the words behind them */
  int64_t q0 = w0 + (int64_t)((4u - (unsigned)(((uintptr_t)(w + w0) >> 2) & 3u)) & 3u);
  if (q0 > w1) q0 = w1;
  const int64_t nq = (w1 - q0) >> 2, q1 = q0 + 4 * nq;
  for (int64_t q = w0 + tid; q < q0; q += nthreads) w[q] = 0u;
  d2d_restore_quad *v = (d2d_restore_quad *)(w + q0);
  const d2d_restore_quad zero = {0u, 0u, 0u, 0u};
  for (int64_t q = tid; q < nq; q += nthreads) v[q] = zero;
  for (int64_t q = q1 + tid; q < w1; q += nthreads) w[q] = 0u;
}

#endif /* D2D_RESTORE_IMPL_H */
