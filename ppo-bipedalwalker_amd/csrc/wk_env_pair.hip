// wk_env_pair.hip -- the flat-floor pair kernels (k_env_side<..., 1, false>: a lane pair per
// walker, the headline rollout).  Built with the physics flags and the max-ILP scheduler (Makefile).
//
// They take the polygons' vertices one at a time instead of in v_pk_*_f32 pairs (wk_device.h,
// WK_VERTEX_PACKED): the same operations, rollout -1.4 % at 65,536 walkers.  The quad kernels
// (wk_env_quad.hip) measured 9 % slower that way and keep the pairs; so do the rough-floor side
// kernels (wk_env_side_rough.hip: its quad kernel +9 %, its pair kernel -1.3 %, one unit) and
// every other kernel (profiles/box_carry_ab.txt).
#ifndef WK_VERTEX_PACKED
#define WK_VERTEX_PACKED 0
#endif
#include "wk_env_side.h"

namespace wk {
void launch_side_pair(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) { launch_side<1, false>(mode, P, A, s); }
}  // namespace wk
RP_HOST_READER  // (probe builds only, wk_region_prof.h)
