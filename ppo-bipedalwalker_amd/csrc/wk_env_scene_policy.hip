// wk_env_scene_policy.hip -- k_env_scene with the fused policy (plain / recording) on the flat
// floor.
#include "wk_env_scene.h"

namespace wk {
void launch_env_scene_policy(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                             hipStream_t s) { scene_policy<false>(mode, P, A, S, s); }
}  // namespace wk
