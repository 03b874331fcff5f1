// wk_env_quad.hip -- the flat-floor quad kernels (k_env_side<..., 2, false>: a lane quad per
// walker, the 8,192-walker shard).  No source-level switch; its own unit because it is built with
// the default scheduler, not max-ILP (Makefile, profiles/r06_sched_ab.txt).
#include "wk_env_side.h"

namespace wk {
void launch_side_quad(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) { launch_side<2, false>(mode, P, A, s); }
}  // namespace wk
