/*
 * d2d_render_hooks.h — test hook of the renderer (libd2d_render.so), apart from the surface of d2d_render.h as d2d_hooks.h is from
 * d2d.h: the rasteriser of d2d_render_frame over a caller-made display list and a caller-made cell layer, so that the tests reach
 * shapes an episode never produces.
 */
#ifndef D2D_RENDER_HOOKS_H
#define D2D_RENDER_HOOKS_H

#include <stdint.h>

#include "d2d_render.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct d2d_render_raster_call {
  const d2d_render_item *items; /* [S][cap] */
  const int32_t *count;         /* [S] items in use, 0 .. cap */
  const uint8_t *cells;         /* [S][W][H] grid codes, row-major */
  int16_t *bbox;                /* [S][cap][4] scratch the call fills */
  uint8_t *frame;               /* [S][Hf][Wf][3] */
  int32_t S, cap, W, H;         /* W = ceil(W_px / scale), H = ceil(H_px / scale) cells at least */
  int32_t W_px, H_px, scale, downsample;
} d2d_render_raster_call;

/* frame[k] = the raster of list k over cell layer k, by the rules of d2d_render.h.  Two launches (the boxes, the frame). */
int d2d_render_raster(const d2d_render_raster_call *call, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_RENDER_HOOKS_H */
