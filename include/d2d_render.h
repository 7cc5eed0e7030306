/*
 * d2d_render.h — C ABI of the renderer (libd2d_render.so): the picture Drone2DEnv2.render draws (envs/drone_v2.py:263-303), for any
 * set of slots of a batch, as a display list and as uint8 frames that stay on the device.
 *
 * Two halves.
 *
 * 1. THE DISPLAY LIST is the reference's own draw calls behind the cell layer, in its order, every number the float64 the reference
 *    passes to pygame.  One d2d_render_item per call; pygame.draw.lines over n points is n - 1 LINE items.  Per slot, in order:
 *      ARC   (100,100,100) width 2   rect = [x - R, y - R, 2 R, 2 R], start = radians(yaw - range / 2), stop = radians(yaw + range / 2)
 *                                    (utils.py:788-796; R = drone_view_depth, range = drone_view_range in degrees)
 *      LINE  (100,100,100) width 2   (x, y) -> (x + R cos(stop), y - R sin(stop)), then the same with start      (utils.py:797-800)
 *      LINE  (100,100,100) width 2   (x - dx, y - dy) -> (x + dx, y + dy) and (x - dy, y + dx) -> (x + dy, y - dx), with
 *                                    dx = 5 cos(radians(yaw + 45)), dy = -5 sin(radians(yaw + 45))                 (utils.py:805-810)
 *      DISC  (100,100,100) r 3.5     at int() of the four arm ends, in the order of utils.py:814-817
 *      DISC  (130,130,130)           every pillar (x, y, r)                                                     (drone_v2.py:269-270)
 *      LINE  (0,0,0) width 2         the stored trajectory's positions joined, if there is more than one        (drone_v2.py:272-273)
 *      per agent k: DISC at rint(position), r = int(round(radius)), (130,176,210) if tracker k is active else (200,36,35);
 *                   LINE (53,53,53) width 2 from rint(position) to rint(position + velocity)                    (drone_v2.py:277-282)
 *      POLY  (0,0,150)               the ten star points around the target, radii drone_radius and 0.5 drone_radius (utils.py:31-51)
 *    radians(a) is a * (pi / 180), the product Python forms; cos / sin are the host libm's bits (csrc/d2d_sincos.h); int() truncates;
 *    rint and round go to the nearest integer, halves to even; the star's sines and cosines, which are constants, come from the
 *    caller (d2d_render_call.star, from the host's math.sin / math.cos).  velocity is agent_vel where the caller has one (RVO), else
 *    the preferred velocity every CVM step assigns (drone_v2.py:178) -- 0 for the first n_seeded agents of a slot whose step counter
 *    is 0, which the reference constructs at rest (drone_v2.py:30).  The stored trajectory is the caller's traj / traj_len where
 *    given, else positions [head, stored) of the device planner's plan_traj / plan_hdr where given, else there is none (NoMove,
 *    Jerk_Primitive, whose trajectory is empty behind every step).
 *    Not drawn: text and covariance ellipses (commented out in the reference), MPC's future_trajectory, the group_id < 0 rectangles.
 *    A slot whose items would not fit `cap` gets status D2D_RENDER_OVERFLOW and count 0: nothing partial.
 *
 * 2. THE FRAME is the list rasterised over the cell layer by the rules below.  They are this project's own: pygame's pixels for round
 *    shapes are not claimed.  All arithmetic is IEEE-754 binary64, one operation per operator (-ffp-contract=off), in the order written.
 *
 *    The sample point of full-resolution pixel (x, y), x to the right, y down, is the point (x, y) itself, x in [0, W_px), y in
 *    [0, H_px).  frame[v][u] is pixel (u d, v d) for the integer downsample d >= 1: the frame is full[::d, ::d], Hf = ceil(H_px / d)
 *    rows of Wf = ceil(W_px / d) pixels of 3 bytes (r, g, b).
 *
 *    Cell layer.  The pixel starts as the colour of cell (x // scale, y // scale) of the drone's map: (100,100,100) for OCCUPIED,
 *    (200,200,200) for UNOCCUPIED and DYNAMIC, (240,240,240) for UNEXPLORED and any other byte, and for a pixel beyond the last cell
 *    (a map size that is no multiple of the scale).  This is the reference's rectangles.
 *    Then the items are applied in list order; an item that covers the pixel replaces its colour, so the last one wins.
 *
 *    DISC (cx, cy, r) covers (x, y) iff  dx dx + dy dy <= r r  with dx = x - cx, dy = y - cy (the sum as written: two products, one
 *    addition).
 *    LINE of width w from a to b is the capsule of radius h = w / 2.  With apx = x - ax, apy = y - ay, abx = bx - ax, aby = by - ay,
 *    t = apx abx + apy aby, l2 = abx abx + aby aby, h2 = h h:
 *      l2 == 0 or t <= 0:  the disc test at a with r r = h2;      t >= l2:  the disc test at b with r r = h2;
 *      otherwise  c c <= h2 l2  with c = abx apy - aby apx.
 *    ARC (rect, start, stop, then cs = cos(start), ss = sin(start), ce = cos(stop), se = sin(stop), range in degrees: geom[6..10])
 *    has its centre at (rect.x + rect.w / 2, rect.y + rect.h / 2) and outer radius R = rect.w / 2.  With dx = x - cx, ey = -(y - cy)
 *    (the screen's y points down), q = dx dx + ey ey and ri = R - w:  the ring test is  ri ri <= q <= R R  (ri < 0 counts as 0).
 *    The wedge, with  a = cs ey - ss dx  (left of the start edge when >= 0) and  b = ce ey - se dx  (right of the stop edge when <= 0):
 *      range >= 360: every direction;   range <= 180: a >= 0 AND b <= 0;   otherwise: a >= 0 OR b <= 0.
 *    The pixel is covered iff both tests hold.
 *    POLY over points p0 .. p(n-1) (3 <= n <= 10; edges pj -> pi for i = 0 .. n - 1 with j = i - 1, and j = n - 1 for i = 0) is the
 *    crossing-number rule: an edge counts iff (yi > y) != (yj > y) and, with  lhs = (x - xi)(yj - yi)  and  rhs = (xj - xi)(y - yi):
 *    lhs < rhs when yj - yi > 0, lhs > rhs when yj - yi < 0.  The pixel is covered iff an odd number of edges count.
 *
 * Conventions as in d2d.h: plain C, the caller owns all memory, DEVICE pointers, every launch asynchronous on the caller's stream, no
 * hidden allocation; 0 or a negative error (-1 NULL pointer or bad argument, -2 another D2D_ABI_VERSION in the cfg, -3 HIP launch
 * error, -4 a size the launch cannot hold) with a thread-local message and no launch.  The launches read d2d_state.drone, agents,
 * active, target, counters and dmap and the call's inputs; they write the call's items, bbox, count, status and frame, nothing else.
 */
#ifndef D2D_RENDER_H
#define D2D_RENDER_H

#include <stdint.h>

#include "d2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_RENDER_VERSION 1

#define D2D_RK_DISC 1 /* geom: cx, cy, r */
#define D2D_RK_LINE 2 /* geom: ax, ay, bx, by */
#define D2D_RK_ARC 3  /* geom: rect x, y, w, h, start, stop (radians), then cos(start), sin(start), cos(stop), sin(stop), range (degrees) */
#define D2D_RK_POLY 4 /* geom: npts points x, y */
#define D2D_RENDER_GEOM 20
#define D2D_RENDER_OK 0
#define D2D_RENDER_OVERFLOW 1
#define D2D_RENDER_BAD_SLOT 2 /* a chosen slot outside [0, cfg.B): nothing of it is read, its list is empty and its frame UNEXPLORED */
#define D2D_RENDER_FIXED 10  /* items of every slot: the arc, 4 lines, 4 rotor discs, the star */
#define D2D_RENDER_MAX_DOWNSAMPLE 64

/* one draw call: 176 bytes */
typedef struct d2d_render_item {
  int32_t kind;   /* D2D_RK_* */
  uint8_t rgb[3];
  uint8_t npts;   /* POLY: its points; else 0 */
  double width;   /* LINE, ARC; else 0 */
  double geom[D2D_RENDER_GEOM];
} d2d_render_item;

/* items of a slot with P pillars, N agents and a trajectory of at most K positions */
#define D2D_RENDER_CAP(P, N, K) (D2D_RENDER_FIXED + (P) + 2 * (N) + ((K) > 1 ? (K) - 1 : 0))

typedef struct d2d_render_call {
  const int32_t *slots;     /* [S] the slots to draw, each in [0, cfg.B); repeats and any order are fine */
  const int32_t *pillars;   /* [B][P][3] x, y, r; NULL with P == 0 */
  const double *agent_vel;  /* [B][2][N] Agent.velocity (RVO), or NULL: the preferred velocity (CVM) */
  const double *plan_traj;  /* [B][plan_cap][4] d2d_plan.traj, or NULL */
  const int32_t *plan_hdr;  /* [B][2] d2d_plan.traj_hdr */
  const double *traj;       /* [S][K][2] the caller's trajectory positions per CHOSEN slot, or NULL; takes the place of plan_traj */
  const int32_t *traj_len;  /* [S] positions of it in use, 0 .. K */
  d2d_render_item *items;   /* [S][cap] */
  int16_t *bbox;            /* [S][cap][4] x0, y0, x1, y1: full-resolution pixels an item can cover, cut to the frame (x0 > x1: none) */
  int32_t *count;           /* [S] */
  uint8_t *status;          /* [S] D2D_RENDER_OK / D2D_RENDER_OVERFLOW / D2D_RENDER_BAD_SLOT */
  uint8_t *frame;           /* [S][Hf][Wf][3]; d2d_render_list does not look at it */
  int32_t S, P, K, plan_cap;
  int32_t cap;              /* >= 1 */
  int32_t n_seeded;         /* agents constructed at rest (drone_v2.py:28-47) */
  int32_t downsample;       /* 1 .. D2D_RENDER_MAX_DOWNSAMPLE */
  int32_t reserved;
  double view_range;        /* drone_view_range, degrees */
  double star[20];          /* sin(pi / 5 * i), cos(pi / 5 * i) for i = 0 .. 9 */
} d2d_render_call;

int d2d_render_version(void);
const char *d2d_render_last_error(void);

/* The display lists of the S chosen slots, one wave per chosen slot: writes items, bbox, count and status.  S == 0: nothing to do. */
int d2d_render_list(const d2d_cfg *cfg, const d2d_state *st, const d2d_render_call *call, void *stream);

/* The frames of the S chosen slots from the lists d2d_render_list left in the call's buffers and from d2d_state.dmap (either grid
 * layout), one workgroup per (slot, tile of 128 x 32 frame pixels).  cfg.scale, W_px and H_px must be whole numbers (-4 otherwise). */
int d2d_render_frame(const d2d_cfg *cfg, const d2d_state *st, const d2d_render_call *call, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_RENDER_H */
