/*
 * d2d_capture.h — the selection rule of include/d2d_capture.h, said once for the device kernel (d2d_render.hip) and for host builds:
 * the kind of a finished slot, whether it matches, and how many of a call's matches are accepted.  Integer work only.
 */
#ifndef D2D_CAPTURE_IMPL_H
#define D2D_CAPTURE_IMPL_H

#include <stdint.h>

#include "../../../include/d2d_capture.h"

#ifndef D2D_RENDER_QUAL
#define D2D_RENDER_QUAL static inline
#endif

/* D2D_CAPTURE_* of a slot from its flag bytes and its state machine's state, the conditions tested in the header's order */
D2D_RENDER_QUAL int d2d_capture_kind(int collision, int dead_lock, int freezing, int sm) {
  return collision == 1 ? D2D_CAPTURE_STATIC : collision == 2 ? D2D_CAPTURE_DYNAMIC : dead_lock ? D2D_CAPTURE_DEAD_LOCK
       : freezing ? D2D_CAPTURE_FREEZING : sm == D2D_SM_GOAL_REACHED ? D2D_CAPTURE_GOAL : D2D_CAPTURE_OTHER;
}

D2D_RENDER_QUAL int d2d_capture_matches(int done, int episode, int steps, int kind, uint32_t kinds) {
  return done != 0 && episode >= 0 && steps > 0 && ((kinds >> (kind - 1)) & 1u) != 0;
}

/* the gallery rows a call may still fill: ranks r < room are accepted (with r < S) */
D2D_RENDER_QUAL long long d2d_capture_room(long long taken, long long capacity) {
  return taken < 0 || taken >= capacity ? 0 : capacity - taken;
}

#endif /* D2D_CAPTURE_IMPL_H */
