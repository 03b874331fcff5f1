// wk_env_side_rough.hip -- RoughFloor on the pair and quad mappings (k_env_side<..., true>).
// Built with the physics flags and the max-ILP scheduler (Makefile).
//
// These kernels keep the compiler's own form of the rotation's Horner steps (wk_sincos_small.h):
// with the scalar-constant steps the rough quad kernel measured 0.4-0.6 % slower at the
// 8,192-walker shard, with the plain steps and the other copy cuts 0.3 % faster than before
// (profiles/copy_cuts_ab.txt).  The same FMAs either way.
#define WK_SC_PLAIN_FMA 1
#include "wk_env_side.h"

namespace wk {
void launch_side_pair_rough(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) { launch_side<1, true>(mode, P, A, s); }
void launch_side_quad_rough(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) { launch_side<2, true>(mode, P, A, s); }
}  // namespace wk
