// wk_env_scene_given_rough.hip -- k_env_scene with given actions (plain / traced) on the rough
// floor.
#include "wk_env_scene.h"

namespace wk {
void launch_env_scene_given_rough(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                                  hipStream_t s) { scene_given<true>(mode, P, A, S, s); }
}  // namespace wk
