/* Host build of csrc/d2d_plan_spec.h for tests/test_plan_spec_cpu.py: the match functions the host dispatch of d2d_closed_loop calls, and
 * the apply functions the specialised kernels run on their own copies, as plain C entry points. */
#include "d2d_plan_spec.h"

extern "C" {
int plan_spec_geometry_matches(const d2d_cfg *c) { return spec_default_matches(*c) ? 1 : 0; }
void plan_spec_geometry_apply(d2d_cfg *c) { spec_default_apply(*c); }
int plan_spec_matches(const d2d_cfg *c, const d2d_plan *p) { return plan_default_matches(*c, *p) ? 1 : 0; }
void plan_spec_apply(d2d_plan *p) { plan_default_apply(*p); }
int plan_spec_sizeof_cfg(void) { return (int)sizeof(d2d_cfg); }
int plan_spec_sizeof_plan(void) { return (int)sizeof(d2d_plan); }
}
