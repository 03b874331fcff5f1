// wk_env_lane.h -- the one-lane and 16-lane-row mapping of the env-step (k_env_step): the whole
// walker in every lane of its row, the scalar and row-parallel policy, and env_frames, the frame
// loop of Environment.Update that k_env_step and k_env_scene (wk_env_scene.h) share.
#pragma once
#include "wk_env_pairs.h"
#include "wk_sample.h"

namespace wk {

// one substep of Environment.StepObjects (:130-142); ec: event counters (counting replay)
template <bool TRACE, int L, bool ROUGH>
DEV void substep(EnvState& s, const Mat& mp, const Mat& mb, float dt, float adx, float ady,
                 PairTraceDev* tr, int sub, const float* ter, uint32_t* ec = nullptr) {
  // joints: [bodyJointLeft, bodyJointRight, leftJoint, rightJoint] (Walker.cs:182-187)
  joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.llu, s.dllu, mp, tr, 0, ec);
  joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.rlu, s.drlu, mp, tr, 1, ec);
  joint_step<6, 6, 2, 3, TRACE>(s.llu, s.dllu, mp, s.lll, s.dlll, mp, tr, 2, ec);
  joint_step<6, 6, 2, 3, TRACE>(s.rlu, s.drlu, mp, s.rll, s.drll, mp, tr, 3, ec);
  // bodies in list order; the floor's own step is a no-op (static, zero velocity).
  // Episode 0 lists the floor last, every later episode first (Walker.cs:212-234):
  // that only changes the order of each leg segment's candidate pairs.
  integrate(s.lll, s.dlll, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) floor_pairs<6, TRACE, L, ROUGH>(s.lll, s.dlll, mp, s.clll, tr, 1, sub, ter, ec);
    else resolve_pair<6, 6, false, TRACE, L>(s.lll, s.dlll, mp, s.llu, s.dllu, mp, s.clll, tr, 0, sub, nullptr, ec);
  }
  integrate(s.llu, s.dllu, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) floor_pairs<6, TRACE, L, ROUGH>(s.llu, s.dllu, mp, s.cllu, tr, 3, sub, ter, ec);
    else resolve_pair<6, 6, false, TRACE, L>(s.llu, s.dllu, mp, s.lll, s.dlll, mp, s.cllu, tr, 2, sub, nullptr, ec);
  }
  integrate(s.body, s.dbody, dt, adx, ady);
  floor_pairs<5, TRACE, L, ROUGH>(s.body, s.dbody, mb, s.cbody, tr, 4, sub, ter, ec);
  integrate(s.rll, s.drll, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) floor_pairs<6, TRACE, L, ROUGH>(s.rll, s.drll, mp, s.crll, tr, 6, sub, ter, ec);
    else resolve_pair<6, 6, false, TRACE, L>(s.rll, s.drll, mp, s.rlu, s.drlu, mp, s.crll, tr, 5, sub, nullptr, ec);
  }
  integrate(s.rlu, s.drlu, dt, adx, ady);
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    if ((q == 0) == s.post) floor_pairs<6, TRACE, L, ROUGH>(s.rlu, s.drlu, mp, s.crlu, tr, 8, sub, ter, ec);
    else resolve_pair<6, 6, false, TRACE, L>(s.rlu, s.drlu, mp, s.rll, s.drll, mp, s.crlu, tr, 7, sub, nullptr, ec);
  }
  if (ec) ec[EV_SUBSTEPS]++;
}

// ---------------- policy (fused, weights read with wave-uniform scalar loads) ----------
// DenseLayer.FeedForward (DenseLayer.cs:82-98): z_j = (sum_k W[j][k] x[k], in order) + b_j
DEV void actor_mean(const float* __restrict__ W, const float s[12], float mean[4]) {
  float h1[64];
#pragma unroll
  for (int j = 0; j < 64; j++) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; k++) acc = acc + W[OFF_A_W1 + j * 12 + k] * s[k];
    float z = acc + W[OFF_A_B1 + j];
    h1[j] = net_maxf(0.2f * z, z);
  }
  float z3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
  for (int j = 0; j < 64; j++) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 64; k++) acc = acc + W[OFF_A_W2 + j * 64 + k] * h1[k];
    float z = acc + W[OFF_A_B2 + j];
    float h2 = net_maxf(0.2f * z, z);
#pragma unroll
    for (int d = 0; d < 4; d++) z3[d] = z3[d] + W[OFF_A_W3 + d * 64 + j] * h2;
  }
#pragma unroll
  for (int d = 0; d < 4; d++) mean[d] = tanhf(z3[d] + W[OFF_A_B3 + d]);
}

DEV float critic_value(const float* __restrict__ W, const float s[12]) {
  float v = 0.0f;
#pragma unroll 4
  for (int j = 0; j < 64; j++) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; k++) acc = acc + W[OFF_C_W1 + j * 12 + k] * s[k];
    float z = acc + W[OFF_C_B1 + j];
    float h = net_maxf(0.2f * z, z);
    v = v + W[OFF_C_W2 + j] * h;
  }
  return v + W[OFF_C_B2];
}

// Row-parallel policy for L = 16 lanes per walker: lane `sub` owns neurons 4*sub..4*sub+3
// of every 64-wide layer (each neuron's sum stays sequential in k, so the values are
// bit-identical to actor_mean / critic_value); activations cross lanes through a
// 192-float LDS slice per walker.  Lanes 0..3 own one action dimension each (output
// neuron, Philox draw, log-density), lane 4 the critic output; results are broadcast
// back to the row.
DEV void policy_row(const EnvParams& P, const float* __restrict__ W, float lp_const,
                    uint32_t gid, uint32_t t, const float obs[12], int sub, int row_base,
                    float* __restrict__ h, bool want_value, float act[4], float logp[4],
                    float& value) {
  float* h1 = h;
  float* h2 = h + 64;
  float* hc = h + 128;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int j = sub * 4 + q;
    float za = 0.0f, zc = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      za = za + W[OFF_A_W1 + j * 12 + k] * obs[k];
      zc = zc + W[OFF_C_W1 + j * 12 + k] * obs[k];
    }
    za = za + W[OFF_A_B1 + j];
    zc = zc + W[OFF_C_B1 + j];
    h1[j] = net_maxf(0.2f * za, za);
    hc[j] = net_maxf(0.2f * zc, zc);
  }
  wave_lds_sync();
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int j = sub * 4 + q;
    float z = 0.0f;
#pragma unroll 16
    for (int k = 0; k < 64; k++) z = z + W[OFF_A_W2 + j * 64 + k] * h1[k];
    z = z + W[OFF_A_B2 + j];
    h2[j] = net_maxf(0.2f * z, z);
  }
  wave_lds_sync();
  // output neurons: lanes 0..3 actor (W3 row d on h2), lane 4 critic (Wc2 on hc)
  const int d = sub & 3;
  const bool vlane = sub == 4;
  const float* wrow = vlane ? (W + OFF_C_W2) : (W + OFF_A_W3 + d * 64);
  const float* xin = vlane ? hc : h2;
  float zo = 0.0f;
#pragma unroll 16
  for (int k = 0; k < 64; k++) zo = zo + wrow[k] * xin[k];
  zo = zo + (vlane ? W[OFF_C_B2] : W[OFF_A_B3 + d]);
  const float mean = tanhf(zo);
  // SampleActions for dimension d (PPOAgent.cs:381-398; NormalDistribution.cs:12-32)
  const float PI_F = 3.14159265358979323846f;
  U4 o = philox(P.seed, gid, t, (uint32_t)d, ST_ACT);
  float u1 = next_double_f(o.x, o.y);
  const float u2 = next_double_f(o.z, o.w);
  if (u1 == 0.0f) u1 = 1.0f;
  const float zn = sqrtf(-2.0f * logf(u1)) * sinf(2.0f * PI_F * u2);
  const float a = mean + (P.std_ * zn);
  float fraction = (a - mean) / P.std_;
  fraction *= fraction;
  fraction /= 2.0f;
  const float lp = lp_const - fraction;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    act[q] = __shfl(a, row_base + q);
    logp[q] = __shfl(lp, row_base + q);
  }
  value = want_value ? __shfl(zo, row_base + 4) : 0.0f;
  wave_lds_sync();  // the slice is rewritten by the next env-step
}

// The frame loop of Environment.Update (Environment.cs:64-180), A.k_steps env-steps of walker e
// held in s: the one text of an env-step for k_env_step and k_env_scene (wk_env_scene.h), which
// keep their own preamble and epilogue and pass their substep of StepObjects as
// step(PairTraceDev*), a force-inlined lambda (a plain one stays an out-of-line call).
// PACE: the pacing call (not in the scene kernel); COUNT: the counting replay's counters ec.
// k_env_side restates this loop in its own shape.
template <bool POLICY, bool RECORD, bool TRACE, int L, bool COUNT, bool PACE, typename Step>
DEV void env_frames(const EnvParams& P, const StepArgs& A, EnvState& s, int e, int sub, float dx,
                    float* pol_lds, uint32_t& t, uint32_t& fault, uint32_t* ec, Step step) {
  const int n = P.n_env;
  const bool leader = sub == 0;
  const uint32_t gid = (uint32_t)(P.env_offset + e);
#pragma unroll 1
  for (int k = 0; k < A.k_steps; k++) {
    float a[4], lp[4], obs[12];
    if (PACE && A.pace) pace_partner(A.pace, A.pace_seq, k);  // (lane 0 always holds a walker)
    if (POLICY) {
      get_obs(s, obs);
      float v = 0.0f;
      if constexpr (L == 16) {
        policy_row(P, A.W, A.lp_const, gid, t, obs, sub, threadIdx.x & ~15,
                   pol_lds + (threadIdx.x >> 4) * 192, RECORD, a, lp, v);
      } else {
        float mean[4];
        actor_mean(A.W, obs, mean);
        sample_actions(P, A.lp_const, gid, t, mean, a, lp);
        if (RECORD) v = critic_value(A.W, obs);
      }
      if (RECORD) {
        if (leader) {
          const size_t idx = (size_t)(A.t0 + k) * n + e;
#pragma unroll
          for (int i = 0; i < 12; i++) A.traj_s[idx * 12 + i] = obs[i];
#pragma unroll
          for (int d = 0; d < 4; d++) {
            A.traj_a[idx * 4 + d] = a[d];
            A.traj_lp[idx * 4 + d] = lp[d];
          }
          A.traj_v[idx] = v;
        }
      }
    } else {
#pragma unroll
      for (int d = 0; d < 4; d++) a[d] = A.actions[((size_t)k * n + e) * 4 + d];
    }
    // Environment.Update (:71-78)
    s.steps++;
    float ac[4];
#pragma unroll
    for (int d = 0; d < 4; d++) ac[d] = clip1(a[d]);
    // Joint.SetTorque on joints [Body-LLU, Body-RLU, LLU-LLL, RLU-RLL]: child w += 5*change
    {
      float c;
      c = ac[0] - s.torque[0]; s.torque[0] = ac[0]; s.dllu.w = s.dllu.w + c * 5.0f;
      c = ac[1] - s.torque[1]; s.torque[1] = ac[1]; s.drlu.w = s.drlu.w + c * 5.0f;
      c = ac[2] - s.torque[2]; s.torque[2] = ac[2]; s.dlll.w = s.dlll.w + c * 5.0f;
      c = ac[3] - s.torque[3]; s.torque[3] = ac[3]; s.drll.w = s.drll.w + c * 5.0f;
    }
    // StepObjects
    const uint32_t lf0 = COUNT ? ec[EV_AABB_LF] : 0u, ll0 = COUNT ? ec[EV_SAT_LL] : 0u;
#pragma unroll 1
    for (int it = 0; it < P.iterations; it++) {
      PairTraceDev* tr = nullptr;
      if (TRACE && leader) {
        tr = A.trace + ((size_t)e * P.iterations + it);
        PairTraceDev z = {};
        *tr = z;
      }
      step(tr);
    }
    if constexpr (COUNT) {
      ec[EV_ENV_STEPS]++;
      ec[EV_STEPS_LF] += ec[EV_AABB_LF] != lf0 ? 1u : 0u;
      ec[EV_STEPS_SATLL] += ec[EV_SAT_LL] != ll0 ? 1u : 0u;
    }
    // Walker.Update
    s.prevx = s.posx; s.prevy = s.posy;
    s.posx = s.body.cx; s.posy = s.body.cy;
    if (s.cbody || s.cllu || s.crlu) s.terminal = true;
    float reward;
    const bool terminal = frame_outcome(P, s, reward);
    if (!state_finite(s)) fault |= 1u;
    if (A.pos_out && leader) {
      A.pos_out[((size_t)k * n + e) * 2] = s.posx;
      A.pos_out[((size_t)k * n + e) * 2 + 1] = s.posy;
    }
    if (terminal) {  // Walker.Reset (scene props keep their state and list positions)
      int ep = s.episodes + 1;
      make_template(s, dx);
      s.post = true;
      s.episodes = ep;
      if constexpr (COUNT) ec[EV_RESETS]++;
    }
    if (leader) {
      if (A.obs_out) {
        get_obs(s, obs);
#pragma unroll
        for (int i = 0; i < 12; i++) A.obs_out[((size_t)k * n + e) * 12 + i] = obs[i];
      }
      if (A.rew_out) A.rew_out[(size_t)k * n + e] = reward;
      if (A.done_out) A.done_out[(size_t)k * n + e] = terminal ? 1 : 0;
      if (RECORD) {
        const size_t idx = (size_t)(A.t0 + k) * n + e;
        A.traj_r[idx] = reward;
        A.traj_d[idx] = terminal ? 1 : 0;
      }
    }
    t++;
  }
}

// L lanes per walker (a "row"): the Gauss-Seidel chain runs replicated in every lane of
// the row (bit-identical state), SAT axes are split one per lane (sat_row); lane 0 of
// the row owns all stores.  L = 1 is the plain one-walker-per-lane mapping.
// COUNT (one lane per walker, given actions): the counting replay -- the same
// physics with per-lane event counters summed into A.counts (SURVEY 8(d) F_counted).
// The kernel's own text is the preamble (the terrain column, the state, the materials, the
// counters) and the epilogue (the state, rng_t, the fault row, the counts' wave sums); the
// env-steps between them are env_frames over substep<TRACE, L, ROUGH>.
template <bool POLICY, bool RECORD, bool TRACE, int L, bool ROUGH, bool COUNT = false>
__global__ __launch_bounds__(64) WK_ENV_WPE void k_env_step(EnvParams P, StepArgs A) {
  static_assert(!COUNT || (L == 1 && !POLICY && !TRACE), "counting replay");
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = tid / L, sub = tid % L;
  const int n = P.n_env;
  if (e >= n) return;  // whole rows exit together
  const bool leader = sub == 0;
  __shared__ float pol_lds[(L == 16 && POLICY) ? 4 * 192 : 1];
  // the walker's rough-floor heights 800 + Random.Next(0, 100), [draw][walker of block]:
  // each lane writes and later reads only its own walker's column (no barrier needed)
  __shared__ float ter_lds[ROUGH ? 11 * 64 : 1];
  float* ter = ter_lds + (threadIdx.x / L);
  if constexpr (ROUGH) {
#pragma unroll 1
    for (int i = 0; i < 11; i++)
      ter[i * 64] = 800.0f + (float)terrain_draw(P.seed, (uint32_t)(P.env_offset + e), i);
  }
  EnvState s;
  load_state(s, A.st, e, n);
  const float dx = A.dxoff[e];
  const StepConsts C = step_consts(P, A.mat[e]);
  uint32_t t = A.rng_t[e];
  uint32_t fault = 0;
  uint32_t ecnt[NEV];
#pragma unroll
  for (int i = 0; i < NEV; i++) ecnt[i] = 0u;
  uint32_t* const ec = COUNT ? ecnt : nullptr;

  env_frames<POLICY, RECORD, TRACE, L, COUNT, true>(
      P, A, s, e, sub, dx, pol_lds, t, fault, ec, [&](PairTraceDev* tr) __attribute__((always_inline)) {
        substep<TRACE, L, ROUGH>(s, C.mp, C.mb, C.dt, C.adx, C.ady, tr, sub, ter, ec);
      });
  if (leader) {
    store_state(s, A.st, e, n);
    A.rng_t[e] = t;
    if (A.fault_out) A.fault_out[e] |= fault;
  }
  if constexpr (COUNT) {  // wave sums, one 64-bit atomic per counter and wave
#pragma unroll
    for (int i = 0; i < NEV; i++) {
      uint32_t v = ecnt[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(A.counts + i, (unsigned long long)v);
    }
  }
}

// host side: k_env_step is instantiated where these are (wk_env.hip)
template <int L, bool ROUGH>
static void launch_lanes_floor(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) {
  dim3 blk(64), grd((unsigned)(((size_t)P.n_env * L + 63) / 64));
  switch (mode) {
    case 0: hipLaunchKernelGGL((k_env_step<false, false, false, L, ROUGH>), grd, blk, 0, s, P, A); break;
    case 1: hipLaunchKernelGGL((k_env_step<false, false, true, L, ROUGH>), grd, blk, 0, s, P, A); break;
    case 2: hipLaunchKernelGGL((k_env_step<true, false, false, L, ROUGH>), grd, blk, 0, s, P, A); break;
    default: hipLaunchKernelGGL((k_env_step<true, true, false, L, ROUGH>), grd, blk, 0, s, P, A); break;
  }
}
template <int L>
static void launch_lanes(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) {
  if (P.rough) launch_lanes_floor<L, true>(mode, P, A, s);
  else launch_lanes_floor<L, false>(mode, P, A, s);
}
}  // namespace wk
