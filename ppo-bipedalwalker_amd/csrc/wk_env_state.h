// wk_env_state.h -- the fused batched env-step kernels for gfx950: the walker's register state
// and what every kernel family does around its substeps (device side).
//
// One launch runs K whole Environment.Update steps (Environment.cs:64-92) for every
// walker: optional policy sampling (PPOAgent.SampleActions, PPOAgent.cs:381-398),
// Clip + Joint.SetTorque (Environment.cs:78, Joint.cs:56-61), Iterations substeps of
// StepObjects (Environment.cs:126-143: Joint.Step Joint.cs:31-41, RigidBody.Step
// Bodies/RigidBody.cs:54-61 with the AABB broadphase Skeleton.cs:133-140, SAT
// Bodies/Physics/SATCollision.cs:15-104, contact clipping ContactPoints.cs:13-134 and
// impulses Impulses.cs:12-115), Walker.Update (Walker.cs:49-54), CalculateReward
// (Environment.cs:148-154), terminal checks (:106-117), GetState (Walker.cs:132-152)
// and auto-reset (Environment.cs:167-180, Walker.cs:212-223).
//
// All walker state lives in VGPRs for the whole launch; HBM is touched only to load
// and store the 112-float SoA state once per launch and to write per-step outputs.
// Arithmetic is restated op-for-op in IEEE fp32 with -ffp-contract=off so the
// trajectories are bit-identical to the CPU oracle (MonoGame Vector2 semantics:
// v / f == v * (1/f); rotation via (float)cos/sin of the double-promoted angle).
//
// The kernel families on top of it, each instantiated by its own translation unit (wk_env*.hip,
// with that unit's switches and the Makefile's flags for it): wk_env_lane.h (k_env_step: one lane
// or a 16-lane row per walker), wk_env_side.h (k_env_side: a lane pair or quad per walker),
// wk_env_scene.h (k_env_scene: one lane per walker, with scene props); wk_env_pairs.h holds the
// joints and candidate pairs they share.
#pragma once
#include "wk_common.h"
#include "wk_device.h"
#include "wk_kernels.h"

// two waves per SIMD for the one- and 16-lane kernels (three: 168 VGPRs, spills, slower)
#define WK_ENV_WPE __attribute__((amdgpu_waves_per_eu(2, 2)))

namespace wk {

struct EnvState {
  Poly<6> lll, llu, rll, rlu;
  Poly<5> body;
  Dyn dlll, dllu, dbody, drll, drlu;
  bool clll, cllu, cbody, crll, crlu;
  float torque[4];
  float posx, posy, prevx, prevy;
  int steps, episodes;
  bool post, terminal;
};

// Pole.FromSize (Objects/RigidBodies/Pole.cs:18-34) + FindCentroid (Skeleton.cs:100-113)
DEV void make_pole(Poly<6>& p, float cx, float cy) {
  float adjustment = 0.1f * 75.0f;
  float h = adjustment * 3.5f;
  p.x[0] = cx + adjustment; p.y[0] = cy + h;
  p.x[1] = cx;              p.y[1] = cy + h;
  p.x[2] = cx - adjustment; p.y[2] = cy + h;
  p.x[3] = cx - adjustment; p.y[3] = cy - h;
  p.x[4] = cx;              p.y[4] = cy - h;
  p.x[5] = cx + adjustment; p.y[5] = cy - h;
  find_centroid(p);
}

DEV void zero_dyn(Dyn& d) { d.vx = 0.0f; d.vy = 0.0f; d.w = 0.0f; d.th = 0.0f; }

// Walker.CreateCreature / Reset + Environment.InitialState
DEV void make_template(EnvState& s, float dx) {
  float px = 125.0f + dx, py = 800.0f;
  s.body.x[0] = px + 20; s.body.y[0] = py + 20;
  s.body.x[1] = px;      s.body.y[1] = py + 20;
  s.body.x[2] = px - 20; s.body.y[2] = py + 20;
  s.body.x[3] = px - 20; s.body.y[3] = py - 20;
  s.body.x[4] = px + 20; s.body.y[4] = py - 20;
  find_centroid(s.body);
  make_pole(s.llu, px + 0.0f, py + 30.0f);
  make_pole(s.lll, px + 0.0f, py + 60.0f);
  make_pole(s.rlu, px + 0.0f, py + 30.0f);
  make_pole(s.rll, px + 0.0f, py + 60.0f);
  zero_dyn(s.dlll); zero_dyn(s.dllu); zero_dyn(s.dbody); zero_dyn(s.drll); zero_dyn(s.drlu);
  s.clll = s.cllu = s.cbody = s.crll = s.crlu = false;
#pragma unroll
  for (int j = 0; j < 4; j++) s.torque[j] = 0.0f;
  s.steps = 0;
  s.terminal = false;
  // InitialState -> Walker.Update: prev = (125, 800); pos = Body centroid
  s.prevx = px; s.prevy = py;
  s.posx = s.body.cx; s.posy = s.body.cy;
}

template <int N>
DEV void load_poly(Poly<N>& p, const float* __restrict__ st, int b, int e, int n) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    p.x[i] = st[(size_t)e * NSTATE + (b * BSTRIDE + 2 * i)];
    p.y[i] = st[(size_t)e * NSTATE + (b * BSTRIDE + 2 * i + 1)];
  }
  p.cx = st[(size_t)e * NSTATE + (b * BSTRIDE + F_CX)];
  p.cy = st[(size_t)e * NSTATE + (b * BSTRIDE + F_CY)];
}
DEV void load_dyn(Dyn& d, bool& col, const float* __restrict__ st, int b, int e, int n) {
  d.vx = st[(size_t)e * NSTATE + (b * BSTRIDE + F_VX)];
  d.vy = st[(size_t)e * NSTATE + (b * BSTRIDE + F_VY)];
  d.w = st[(size_t)e * NSTATE + (b * BSTRIDE + F_W)];
  d.th = st[(size_t)e * NSTATE + (b * BSTRIDE + F_TH)];
  col = st[(size_t)e * NSTATE + (b * BSTRIDE + F_COL)] != 0.0f;
}
template <int N>
DEV void store_body(const Poly<N>& p, const Dyn& d, bool col, float* __restrict__ st, int b, int e,
                    int n) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    st[(size_t)e * NSTATE + (b * BSTRIDE + 2 * i)] = i < N ? p.x[i < N ? i : 0] : 0.0f;
    st[(size_t)e * NSTATE + (b * BSTRIDE + 2 * i + 1)] = i < N ? p.y[i < N ? i : 0] : 0.0f;
  }
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_CX)] = p.cx;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_CY)] = p.cy;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_VX)] = d.vx;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_VY)] = d.vy;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_W)] = d.w;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_TH)] = d.th;
  st[(size_t)e * NSTATE + (b * BSTRIDE + F_COL)] = col ? 1.0f : 0.0f;
  st[(size_t)e * NSTATE + (b * BSTRIDE + 19)] = 0.0f;
}

DEV void load_state(EnvState& s, const float* __restrict__ st, int e, int n) {
  load_poly(s.lll, st, LLL, e, n);
  load_poly(s.llu, st, LLU, e, n);
  load_poly(s.body, st, BODY, e, n);
  load_poly(s.rll, st, RLL, e, n);
  load_poly(s.rlu, st, RLU, e, n);
  load_dyn(s.dlll, s.clll, st, LLL, e, n);
  load_dyn(s.dllu, s.cllu, st, LLU, e, n);
  load_dyn(s.dbody, s.cbody, st, BODY, e, n);
  load_dyn(s.drll, s.crll, st, RLL, e, n);
  load_dyn(s.drlu, s.crlu, st, RLU, e, n);
#pragma unroll
  for (int j = 0; j < 4; j++) s.torque[j] = st[(size_t)e * NSTATE + (S_TORQUE + j)];
  s.posx = st[(size_t)e * NSTATE + S_POS];
  s.posy = st[(size_t)e * NSTATE + (S_POS + 1)];
  s.prevx = st[(size_t)e * NSTATE + S_PREV];
  s.prevy = st[(size_t)e * NSTATE + (S_PREV + 1)];
  s.steps = (int)st[(size_t)e * NSTATE + S_STEPS];
  s.post = st[(size_t)e * NSTATE + S_POSTRESET] != 0.0f;
  s.terminal = st[(size_t)e * NSTATE + S_TERMINAL] != 0.0f;
  s.episodes = (int)st[(size_t)e * NSTATE + S_EPISODES];
}

DEV void store_state(const EnvState& s, float* __restrict__ st, int e, int n) {
  store_body(s.lll, s.dlll, s.clll, st, LLL, e, n);
  store_body(s.llu, s.dllu, s.cllu, st, LLU, e, n);
  store_body(s.body, s.dbody, s.cbody, st, BODY, e, n);
  store_body(s.rll, s.drll, s.crll, st, RLL, e, n);
  store_body(s.rlu, s.drlu, s.crlu, st, RLU, e, n);
#pragma unroll
  for (int j = 0; j < 4; j++) st[(size_t)e * NSTATE + (S_TORQUE + j)] = s.torque[j];
  st[(size_t)e * NSTATE + S_POS] = s.posx;
  st[(size_t)e * NSTATE + (S_POS + 1)] = s.posy;
  st[(size_t)e * NSTATE + S_PREV] = s.prevx;
  st[(size_t)e * NSTATE + (S_PREV + 1)] = s.prevy;
  st[(size_t)e * NSTATE + S_STEPS] = (float)s.steps;
  st[(size_t)e * NSTATE + S_POSTRESET] = s.post ? 1.0f : 0.0f;
  st[(size_t)e * NSTATE + S_TERMINAL] = s.terminal ? 1.0f : 0.0f;
  st[(size_t)e * NSTATE + S_EPISODES] = (float)s.episodes;
}

// Walker.GetState (Walker.cs:132-152)
DEV void get_obs(const EnvState& s, float o[12]) {
  o[0] = s.body.x[1] / 900.0f;
  o[1] = s.body.y[1] / 500.0f;
  o[2] = s.llu.x[2] / 900.0f;
  o[3] = s.llu.y[2] / 500.0f;
  o[4] = s.rlu.x[2] / 900.0f;
  o[5] = s.rlu.y[2] / 500.0f;
  o[6] = s.dbody.vx / 60.0f;
  o[7] = s.dbody.vy / 60.0f;
  o[8] = s.dlll.th;
  o[9] = s.dllu.th;
  o[10] = s.drll.th;
  o[11] = s.drlu.th;
}

// LDS written by some lanes of a wave and read by others of the same wave (the activations of
// policy_row, the tiles of policy_mfma): ordered within the wave, no block barrier
DEV void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// WK_FAULT_NONFINITE: x * 0 is NaN exactly for a NaN or infinite x, so the sum over every
// vertex, centroid and velocity of the walker stays 0 iff all are finite (once per env-step)
template <int N>
DEV float nonfinite_acc(const Poly<N>& p, const Dyn& d) {
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < N; i++) acc += p.x[i] * 0.0f + p.y[i] * 0.0f;
  return acc + (p.cx * 0.0f + p.cy * 0.0f) + (d.vx * 0.0f + d.vy * 0.0f) + (d.w * 0.0f + d.th * 0.0f);
}
DEV bool state_finite(const EnvState& s) {
  const float acc = nonfinite_acc(s.lll, s.dlll) + nonfinite_acc(s.llu, s.dllu) +
                    nonfinite_acc(s.rll, s.drll) + nonfinite_acc(s.rlu, s.drlu) +
                    nonfinite_acc(s.body, s.dbody);
  return acc == 0.0f;
}

// Pacing of co-resident waves (k_env_side's pair mapping: two 4-wave blocks per CU; k_env_step:
// two 64-lane blocks per SIMD).  The SIMD arbitrates VALU issue between its co-resident waves by
// priority, then age (MI355X_MICROARCH.md, "Two waves per SIMD"): at equal priority the older
// block's waves issue first, so in the 65,536-walker rollout they finished their 64 env-steps in
// ~25 ms while the younger block's waves, left the spare slots, ran on alone for another ~14 ms at
// one wave per SIMD (per-wave clocks, scripts/r06_wave_clock.py, profiles/r06_wave_clock.txt).
// Each wave publishes (launch, env-step) in its SIMD's slot once per env-step -- an atomic max
// from one lane -- and runs at priority 1 while the slot says another wave there is ahead, 0
// otherwise, so the waves keep pace and share the SIMD to the end.  Scheduling only: no result
// depends on it.
DEV void pace_partner(unsigned long long* pace, uint32_t seq, int k) {
  const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);  // HW_ID
  const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // XCC_ID[3:0]
  const uint32_t slot = (((((xcc & 7u) * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u +
                          ((hw >> 8) & 15u)) * 4u) + ((hw >> 4) & 3u);  // (XCC, SE, SH, CU, SIMD)
  const unsigned long long tag = ((unsigned long long)seq << 32) | (uint32_t)k;
  unsigned long long prev = 0;
  if ((threadIdx.x & 63) == 0) prev = atomicMax(&pace[slot], tag);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(prev >> 32), 0);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)prev, 0);
  if ((((unsigned long long)hi << 32) | lo) > tag) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

// What every env-step kernel's substeps take besides the state: the walker's part and torso
// materials (Walker.cs:168) and the substep's time and gravity step, _acceleration * deltaTime
struct StepConsts {
  Mat mp, mb;
  float dt, adx, ady;
};
DEV StepConsts step_consts(const EnvParams& P, int material_id) {
  const MatConst mc = material(material_id);
  const float dt = P.dt_sub;
  return {{mc.inv_mass, 0.001f * mc.inv_mass, mc.restitution, mc.friction},
          {mc.inv_mass, 0.0003f, mc.restitution, mc.friction}, dt, 0.0f * dt, 980.0f * dt};
}

// The outcome of a frame, after Walker.Update has set the position and s.terminal:
// CalculateReward (Environment.cs:148-154) and the terminal checks (:106-117)
DEV bool frame_outcome(const EnvParams& P, const EnvState& s, float& reward) {
  reward = 0.0f;
  float dX = s.posx - s.prevx;
  float yb = s.body.y[1];
  reward = reward + ((dX > 0.0f && ((yb / 500.0f) < 1.6f)) ? dX : 0.0f);
  reward = reward - (((yb / 500.0f) > 1.65f) ? -0.1f : 0.0f);
  bool terminal = false;
  if (s.terminal || s.steps > P.max_timesteps) {
    if (s.terminal) reward -= 40.0f;
    terminal = true;
  }
  if (s.posx > 900.0f) {
    reward += 80.0f;
    terminal = true;
  }
  return terminal;
}

}  // namespace wk
