// wk_sample.h -- the action sampler shared by the fused rollout kernels (wk_env_*.h) and the
// general networks' policy kernel (wk_net.hip): the noise depends on (seed, global env id,
// env-step, dimension) only, never on the network.
#pragma once
#include "wk_common.h"

namespace wk {

// NormalDistribution.BoxMullerTransform (NormalDistribution.cs:12-19) with Philox draws
__device__ __forceinline__ void sample_actions(const EnvParams& P, float lp_const, uint32_t gid, uint32_t t,
                        const float mean[4], float act[4], float logp[4]) {
  const float PI_F = 3.14159265358979323846f;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    U4 o = philox(P.seed, gid, t, (uint32_t)d, ST_ACT);
    float u1 = next_double_f(o.x, o.y);
    float u2 = next_double_f(o.z, o.w);
    if (u1 == 0.0f) u1 = 1.0f;
    float z = sqrtf(-2.0f * logf(u1)) * sinf(2.0f * PI_F * u2);
    act[d] = mean[d] + (P.std_ * z);
  }
#pragma unroll
  for (int d = 0; d < 4; d++) {
    // LogProbabilityDensity (:24-32); lp_const = -ln(std) - ln(sqrt(2 pi)) (host libm)
    float fraction = (act[d] - mean[d]) / P.std_;
    fraction *= fraction;
    fraction /= 2.0f;
    logp[d] = lp_const - fraction;
  }
}

}  // namespace wk
