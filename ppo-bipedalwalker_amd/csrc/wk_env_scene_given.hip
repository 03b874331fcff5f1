// wk_env_scene_given.hip -- k_env_scene with given actions (plain / traced) on the flat floor.
#include "wk_env_scene.h"

namespace wk {
void launch_env_scene_given(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                            hipStream_t s) { scene_given<false>(mode, P, A, S, s); }
}  // namespace wk
