// d2d_stream_count.inc -- cnt = the number of non-zero cells of slot e's dmap, summed over the wave: the body shared as text by
// stream_harvest_kernel (the record's column D2D_STREAM_R_DMAP) and stream_explored_kernel (include/d2d_worlds_turn.h).  Reads st, e,
// lane, W, H and tile of the including kernel.  Row-major: an env's grid starts anywhere (W * H need not be a multiple of 4), so single
// bytes at the two ends, as fill_bytes writes them.  Tiled: an env's grid is whole tiles of 256 bytes, a word lies inside one row of
// one tile, and of its four cells those with j < H of a row i < W count -- the padding is skipped, whatever it holds.
  const int G = d2d_w_grid_bytes(W, H, tile);
  const uint8_t *p = st.dmap + (size_t)e * G;
  int cnt = 0;
  if (!tile) {
    int head = (int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u);
    if (head > G) head = G;
    if (lane < head) cnt += p[lane] != 0;
    const int nw = (G - head) >> 2;
    const uint32_t *w = (const uint32_t *)(p + head);
    for (int q = lane; q < nw; q += WAVE) cnt += nonzero_bytes(w[q], 4);
    const int t0 = head + 4 * nw;
    if (t0 + lane < G) cnt += p[t0 + lane] != 0;
  } else {
    const uint32_t *w = (const uint32_t *)p;        // e * G is a multiple of 256 and the field's base is a word's
    for (int q = lane; q < (G >> 2); q += WAVE) {
      int i, j;
      d2d_w_cell_of(4 * q, W, H, tile, &i, &j);     // the word's first cell; the other three follow it in j
      const int n = i < W ? min(max(H - j, 0), 4) : 0;
      if (n) cnt += nonzero_bytes(w[q], n);
    }
  }
  cnt = wave_sum(cnt);
