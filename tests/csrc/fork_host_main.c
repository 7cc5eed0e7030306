/* Stand-alone driver of tests/csrc/fork_host.c for the sanitizer run of tests/test_fork_host_build.py: reads the handmade cases the
 * test wrote (one item of one launch a line: item index, in_place, B_dst, B_src, row bytes, the two base offsets, the two strides,
 * then src_of), runs the host loop on heap buffers that end exactly where the last slot's row ends -- so a byte read or written
 * outside a named row is the sanitizer's to report -- filled with tests/fork_model.py's pattern, and prints the digest (fork_model.digest) of the
 * destination buffer and the status bytes, which the test compares with the model's.  Exit status 0: every case ran; 1: usage or
 * read error; 2: the entry point refused a case. */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fork/d2d_fork.h"

int fork_host_slots(const d2d_fork_item *items, int32_t n_items, const int32_t *src_of, int32_t B_dst, int32_t B_src, int32_t in_place,
                    uint8_t *status, char *why, int n);

static void fill(uint8_t *p, uint64_t size, uint64_t seed) { /* fork_model.fill */
  for (uint64_t i = 0; i < size; ++i) p[i] = (uint8_t)((i * (7 + 2 * seed) + seed + (i >> 8)) & 0xff);
}

static uint64_t weigh(uint64_t h, const uint8_t *p, uint64_t n, uint64_t at) { /* fork_model.digest: bytes [at, at + n) of the whole */
  for (uint64_t i = 0; i < n; ++i) h += ((uint64_t)p[i] + 1) * ((at + i + 1) * 0x9e3779b97f4a7c15ull);
  return h;
}

static uint64_t extent(int64_t base, int64_t stride, int64_t n, int64_t B) { return (uint64_t)(B ? base + stride * (B - 1) + n : base); }

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 1;
  long long index, in_place, B_dst, B_src, n, db, sb, ds, ss;
  int cases = 0;
  while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", &index, &in_place, &B_dst, &B_src, &n, &db, &sb, &ds, &ss) == 9) {
    int32_t *src_of = (int32_t *)malloc(sizeof(int32_t) * (size_t)(B_dst ? B_dst : 1));
    uint8_t *status = (uint8_t *)malloc((size_t)(B_dst ? B_dst : 1));
    if (!src_of || !status) return 1;
    for (long long e = 0; e < B_dst; ++e) {
      long long v;
      if (fscanf(f, "%lld", &v) != 1) return 1;
      src_of[e] = (int32_t)v;
    }
    memset(status, 0xee, (size_t)B_dst);
    /* malloc aligns to 16: the offsets choose the alignment, and the buffer ends with the last row */
    const uint64_t dn = extent(db, ds, n, B_dst), sn = extent(sb, ss, n, B_src);
    uint8_t *dst = (uint8_t *)malloc(dn ? dn : 1), *src = in_place ? dst : (uint8_t *)malloc(sn ? sn : 1);
    if (!dst || !src) return 1;
    fill(dst, dn, (uint64_t)(2 * index + 1));
    if (!in_place) fill(src, sn, (uint64_t)(2 * index + 2));
    /* the item array holds `index` empty items in front of the one under test, so that it has the index the case names */
    d2d_fork_item *items = (d2d_fork_item *)calloc((size_t)index + 1, sizeof(d2d_fork_item));
    if (!items) return 1;
    const d2d_fork_item it = {dst + db, src + sb, ds, ss, n};
    items[index] = it;
    char why[256];
    const int rc = fork_host_slots(items, (int32_t)index + 1, src_of, (int32_t)B_dst, (int32_t)B_src, (int32_t)in_place, status, why, (int)sizeof why);
    if (rc) {
      fprintf(stderr, "fork_host: case %d: %d %s\n", cases, rc, why);
      return 2;
    }
    printf("%016" PRIx64 "\n", weigh(weigh(0, dst, dn, 0), status, (uint64_t)B_dst, dn));
    free(items);
    if (!in_place) free(src);
    free(dst);
    free(status);
    free(src_of);
    ++cases;
  }
  fclose(f);
  fprintf(stderr, "fork_host ok: %d cases\n", cases);
  return 0;
}
