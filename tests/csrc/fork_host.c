/* Host build of the slot fork's scalar logic (csrc/fork/d2d_fork.h) for tests/test_fork_host_build.py and tests/test_fork_cpu.py: the
 * entry point of include/d2d_fork.h as a loop that plays every workgroup and thread of every destination slot in turn over host
 * memory, and the sizes and constants the ctypes mirror is checked against. */
#include <stddef.h>
#include <stdint.h>
#include "fork/d2d_fork.h"
int fork_host_slots(const d2d_fork_item *items, int32_t n_items, const int32_t *src_of, int32_t B_dst, int32_t B_src, int32_t in_place,
                    uint8_t *status, char *why, int n) {
  const char *text;
  const int rc = d2d_fork_check(items, n_items, src_of, B_dst, B_src, in_place, status, &text);
  int i = 0;
  for (; i + 1 < n && text[i]; ++i) why[i] = text[i];
  if (n > 0) why[i] = 0;
  if (rc) return rc;
  /* the decisions first, as a launch whose workgroups all read src_of before any of them is done would see them; src_of is not
   * written, so any order gives these */
  for (int64_t e = 0; e < B_dst; ++e)
    for (int part = 0; part < D2D_FORK_PARTS; ++part) {
      const int st = d2d_fork_decide(src_of, e, B_src, in_place);
      if (part == 0) status[e] = (uint8_t)st;
      if (st != D2D_FORK_COPIED) continue;
      for (int k = 0; k < n_items; ++k)
        for (int tid = 0; tid < D2D_FORK_BLOCK; ++tid) d2d_fork_copy_row(items + k, k, e, (int64_t)src_of[e], part, tid, D2D_FORK_BLOCK);
    }
  return 0;
}
int fork_host_version(void) { return D2D_FORK_VERSION; }
int fork_host_item_bytes(void) { return (int)sizeof(d2d_fork_item); }
int fork_host_item_offset(int field) {
  switch (field) {
    case 0: return (int)offsetof(d2d_fork_item, dst);
    case 1: return (int)offsetof(d2d_fork_item, src);
    case 2: return (int)offsetof(d2d_fork_item, dst_stride);
    case 3: return (int)offsetof(d2d_fork_item, src_stride);
    case 4: return (int)offsetof(d2d_fork_item, bytes);
    default: return -1;
  }
}
int fork_host_constant(int which) {
  static const int v[] = {D2D_FORK_MAX_ITEMS, D2D_FORK_PARTS, D2D_FORK_SMALL_BYTES, D2D_FORK_LEFT, D2D_FORK_COPIED, D2D_FORK_REFUSED, D2D_FORK_BLOCK};
  return which >= 0 && which < (int)(sizeof v / sizeof v[0]) ? v[which] : -1;
}
