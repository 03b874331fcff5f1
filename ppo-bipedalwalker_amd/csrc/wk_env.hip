// wk_env.hip -- the rollout's entry points: the dispatchers launch_env_step / launch_env_scene
// over the kernel families (the other wk_env_*.hip units, declared in wk_kernels.h), the one- and
// 16-lane kernels (k_env_step, wk_env_lane.h) with the counting replay, and the small kernels
// around a rollout: init, observations, the standalone policy.
#include "wk_env_lane.h"

namespace wk {

// env initialisation: Environment ctor (Environment.cs:39-51) -- episode-0 body order
__global__ void k_env_init(EnvParams P, float* st, const float* dxoff, const uint8_t* mask,
                           int post) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.n_env) return;
  if (mask && !mask[e]) return;
  EnvState s;
  int episodes = post ? (int)st[(size_t)e * NSTATE + S_EPISODES] : 0;
  make_template(s, dxoff[e]);
  s.post = post != 0;
  s.episodes = episodes;
  store_state(s, st, e, P.n_env);
}

__global__ void k_get_obs(EnvParams P, const float* st, float* obs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.n_env) return;
  EnvState s;
  load_state(s, st, e, P.n_env);
  float o[12];
  get_obs(s, o);
  for (int i = 0; i < 12; i++) obs[(size_t)e * 12 + i] = o[i];
}

// standalone policy evaluation (wk_policy_sample / wk_value)
__global__ void k_policy(EnvParams P, const float* __restrict__ W, float lp_const, int n,
                         const float* obs, const int32_t* env_ids, const uint32_t* steps,
                         float* mean_out, float* act_out, float* logp_out, float* v_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s[12];
  for (int k = 0; k < 12; k++) s[k] = obs[(size_t)i * 12 + k];
  if (v_out) {
    v_out[i] = critic_value(W, s);
    return;
  }
  float mean[4], a[4], lp[4];
  actor_mean(W, s, mean);
  uint32_t gid = env_ids ? (uint32_t)env_ids[i] : (uint32_t)(P.env_offset + i);
  uint32_t t = steps ? steps[i] : 0u;
  sample_actions(P, lp_const, gid, t, mean, a, lp);
  for (int d = 0; d < 4; d++) {
    if (mean_out) mean_out[(size_t)i * 4 + d] = mean[d];
    if (act_out) act_out[(size_t)i * 4 + d] = a[d];
    if (logp_out) logp_out[(size_t)i * 4 + d] = lp[d];
  }
}

// host-side launch shims (C++ linkage, used by wk_api_env.cpp)
hipError_t launch_env_scene(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                            hipStream_t s) {
  if (mode <= 1) (P.rough ? launch_env_scene_given_rough : launch_env_scene_given)(mode, P, A, S, s);
  else (P.rough ? launch_env_scene_policy_rough : launch_env_scene_policy)(mode, P, A, S, s);
  return hipGetLastError();
}
hipError_t launch_env_step(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) {
  if (mode == 4) {  // counting replay: one lane per walker, given actions (flat or rough floor)
    if (!A.counts || !A.actions) return hipErrorInvalidValue;
    dim3 blk(64), grd((unsigned)((P.n_env + 63) / 64));
    if (P.rough) hipLaunchKernelGGL((k_env_step<false, false, false, 1, true, true>), grd, blk, 0, s, P, A);
    else hipLaunchKernelGGL((k_env_step<false, false, false, 1, false, true>), grd, blk, 0, s, P, A);
    return hipGetLastError();
  }
  if (P.lanes == 2) (P.rough ? launch_side_pair_rough : launch_side_pair)(mode, P, A, s);
  else if (P.lanes == 4) (P.rough ? launch_side_quad_rough : launch_side_quad)(mode, P, A, s);
  else if (P.lanes == 16) launch_lanes<16>(mode, P, A, s);
  else launch_lanes<1>(mode, P, A, s);
  return hipGetLastError();
}
hipError_t launch_env_init(const EnvParams& P, float* st, const float* dx, const uint8_t* mask,
                           int post, hipStream_t s) {
  hipLaunchKernelGGL(k_env_init, dim3((P.n_env + 255) / 256), dim3(256), 0, s, P, st, dx, mask, post);
  return hipGetLastError();
}
hipError_t launch_get_obs(const EnvParams& P, const float* st, float* obs, hipStream_t s) {
  hipLaunchKernelGGL(k_get_obs, dim3((P.n_env + 255) / 256), dim3(256), 0, s, P, st, obs);
  return hipGetLastError();
}
hipError_t launch_policy(const EnvParams& P, const float* W, float lp_const, int n,
                         const float* obs, const int32_t* env_ids, const uint32_t* steps,
                         float* mean, float* act, float* logp, float* v, hipStream_t s) {
  hipLaunchKernelGGL(k_policy, dim3((n + 63) / 64), dim3(64), 0, s, P, W, lp_const, n, obs,
                     env_ids, steps, mean, act, logp, v);
  return hipGetLastError();
}
}  // namespace wk
