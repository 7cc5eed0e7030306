/* Stand-alone host program around the scalar item logic of d2d_stream_restore (csrc/worlds/d2d_restore.h), for
 * tests/test_action_stream_cpu.py: built with AddressSanitizer and UBSan and run as a child process.  Every workgroup and thread of a
 * slot is played in turn over heap buffers that end exactly where the item's last slot ends, so a byte written or read outside a
 * named range is the sanitizer's to report, and the result is compared with memset / memcpy over a poisoned buffer. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "worlds/d2d_restore.h"

#define POISON 0xA5
#define SLOTS 3

static int run_case(int64_t bytes, int dst_align, int src_align, int kind, int index) {
  const int64_t dst_stride = bytes + 5, src_stride = bytes + 11, dst_off = dst_align, src_off = 7;
  /* the last slot's range ends with the buffer: dst_stride * (SLOTS - 1) + dst_off + bytes */
  const size_t dn = (size_t)(dst_stride * (SLOTS - 1) + dst_off + bytes), sn = (size_t)(src_stride * (SLOTS - 1) + src_off + src_align + bytes);
  uint8_t *raw_d = (uint8_t *)malloc(dn + 8), *raw_s = (uint8_t *)malloc(sn + 8), *want = (uint8_t *)malloc(dn + 8);
  if (!raw_d || !raw_s || !want) return 2;
  /* malloc aligns to 16: the base is a word's, the offsets choose the alignment */
  for (size_t i = 0; i < sn; ++i) raw_s[i] = (uint8_t)(i * 7 + 1);
  memset(raw_d, POISON, dn);
  memset(want, POISON, dn);
  d2d_restore_item it = {raw_d, raw_s, dst_stride, src_stride, dst_off, src_off + src_align, bytes, kind, 0};
  for (int e = 0; e < SLOTS; ++e) {
    if (e == 1) continue; /* a slot that is not refilled keeps its bytes */
    if (kind == D2D_RESTORE_ZERO) memset(want + e * dst_stride + dst_off, 0, (size_t)bytes);
    else if (kind == D2D_RESTORE_COPY) memcpy(want + e * dst_stride + dst_off, raw_s + e * src_stride + src_off + src_align, (size_t)bytes);
    for (int part = 0; part < D2D_RESTORE_PARTS; ++part)
      for (int tid = 0; tid < D2D_RESTORE_BLOCK; ++tid) {
        d2d_restore_apply(&it, index, e, part, tid, D2D_RESTORE_BLOCK);
      }
  }
  int bad = memcmp(raw_d, want, dn) != 0;
  if (bad) fprintf(stderr, "restore_host: bytes %lld dst_align %d src_align %d kind %d index %d\n", (long long)bytes, dst_align, src_align, kind, index);
  free(raw_d);
  free(raw_s);
  free(want);
  return bad;
}

int main(void) {
  /* 1089 = a slot's obs_local, 899 = a 29 x 31 grid; 4096 / 4100 words straddle D2D_RESTORE_SMALL_WORDS; 153600 = the search's nodes */
  static const int64_t sizes[] = {0, 1, 2, 3, 4, 5, 7, 8, 40, 899, 1089, 4096, 4097, 4099, 4100, 4103, 4 * 1024 + 3, 4 * 1025, 4 * 1025 + 6, 32781};
  int cases = 0;
  for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k)
    for (int da = 0; da < 4; ++da)
      for (int sa = 0; sa < 4; ++sa)
        for (int kind = 0; kind < 3; ++kind) { /* 2: an unknown kind writes nothing */
          if (kind != D2D_RESTORE_COPY && sa) continue;
          if (sizes[k] > 5000 && (da > 1 || sa > 1)) continue;
          const int rc = run_case(sizes[k], da, sa, kind, (int)(k + da) % 11);
          if (rc) return rc;
          ++cases;
        }
  if (run_case(153600, 0, 0, D2D_RESTORE_ZERO, 12) || run_case(153600, 3, 1, D2D_RESTORE_COPY, 5)) return 1;
  printf("restore_host ok: %d cases\n", cases + 2);
  return 0;
}
