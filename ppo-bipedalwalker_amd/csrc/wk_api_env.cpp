// wk_api_env.cpp -- the environment's entry points: the env-step launches and their argument
// blocks, wk_step*, the reference's per-body call shape, observations and walker state with its
// guard, body and prop views, scene props, the rollout mapping and the counting replay.
#include <cmath>
#include <cstring>

#include "wk_ctx.h"

// the env-step kernel of the context's mapping; with scene props the one-lane scene kernel.
// The split mappings first order their lanes (WK_ORDER=0 keeps the identity order, for
// measurements).  Flat floor: episode-0 walkers in the last slots (wk_order.hip, before every
// launch; the quad mapping gains 2-3 %, the pair mapping 9.5 %).  Rough floor: the static order by
// start offset (rough_order_upload) -- not the episode-0 partition, which at one wave per SIMD
// gathered the few long-lived episode-0 walkers into one slowest wave (63 -> 74 ms per rollout
// at 8,192 walkers, scripts/r04_rough2.sh).
// The walkers stepped are A's (A.st, A.rng_t) with the prop states `props`; the flat floor's order
// is built from A.st, the records being stepped (the kernels rely on that partition), into `order`
// (3 n cells: the order, then the swap ranks' scratch) with the tile counters `order_cnt`.  The
// pacing tags are the context's whichever walkers are stepped (they pace launches, not walkers).
hipError_t launch_physics(wk_ctx* c, int mode, wk::StepArgs& A, float* props, int32_t* order,
                          uint32_t* order_cnt) {
  if (c->scene.n_props > 0) {
    A.props = props;
    return wk::launch_env_scene(mode, c->P, A, c->scene, c->stream);
  }
  if (order && (c->P.lanes == 2 || c->P.lanes == 4)) {
    if (!c->P.rough) {
      const hipError_t e = wk::launch_walker_order(A.st, c->n, order_cnt, order, order + c->n, c->stream);
      if (e != hipSuccess) return e;
    }
    A.order = order;
  }
  A.pace = c->pace;
  if (c->pace && ++c->pace_seq == 0) {  // (2^32 launches: the tags start over, so clear the slots)
    const hipError_t e = hipMemsetAsync(c->pace, 0, sizeof(unsigned long long) * wk::PACE_SLOTS, c->stream);
    if (e != hipSuccess) return e;
    c->pace_seq = 1;
  }
  A.pace_seq = c->pace_seq;
  return wk::launch_env_step(mode, c->P, A, c->stream);
}
// the context's own walkers (every A built by env_args)
static hipError_t launch_physics(wk_ctx* c, int mode, wk::StepArgs& A) {
  return launch_physics(c, mode, A, c->props, c->order, c->order_cnt);
}

// the env-step kernels' argument block: the four walker arrays ...
static wk::StepArgs env_args(wk_ctx* c) {
  wk::StepArgs A{};
  A.st = c->st; A.dxoff = c->dxoff; A.mat = c->mat; A.rng_t = c->rng_t;
  return A;
}
// ... the six rows the sampling modes record, from row 0 ...
static void set_traj(wk::StepArgs& A, float* s, float* a, float* lp, float* r, uint8_t* d, float* v) {
  A.traj_s = s; A.traj_a = a; A.traj_lp = lp; A.traj_r = r; A.traj_d = d; A.traj_v = v;
  A.t0 = 0;
}
// ... and the policy those modes run; the rows are the context's unless the caller re-points them
wk::StepArgs policy_args(wk_ctx* c) {
  wk::StepArgs A = env_args(c);
  A.W = c->W; A.Wz = c->Wz; A.lp_const = c->lp_const;
  set_traj(A, c->ts, c->ta, c->tlp, c->tr, c->td, c->tv);
  return A;
}

// the seam between the two kernel families: the policy / value kernel (and launch_grad_for, below)
hipError_t launch_policy_for(wk_ctx* c, int n, const float* obs, const int32_t* ids,
                             const uint32_t* steps, float* mean, float* act, float* logp, float* v) {
  return c->general ? wk::launch_net_policy(c->P, c->net_dev, c->act_rows, c->W, c->lp_const, n, obs, ids,
                                            steps, mean, act, logp, v, c->stream)
                    : wk::launch_policy(c->P, c->W, c->lp_const, n, obs, ids, steps, mean, act, logp, v,
                                        c->stream);
}

// The general networks' sampled env-steps (NetworkKernels = 1).  Per env-step: the walkers'
// observations, the policy kernel on them (Philox step = the walker's env-step counter, as in
// the fused kernels), then one env-step of the context's own physics kernel in its
// caller-actions mode -- every mapping, the rough floor, scene props, the lane order and the
// pacing as they are, and the counters advance as in the fused rollout.  Rows [k][n][.] the
// caller does not keep (null) go through one scratch row.
static int net_sampled(wk_ctx* c, int k, float* d_s, float* d_a, float* d_lp, float* d_v, float* d_r,
                       uint8_t* d_d, float* d_obs, float* d_pos, uint32_t* d_fault) {
  const size_t n = c->n;
  float *r_s = nullptr, *r_a = nullptr, *r_lp = nullptr, *r_v = nullptr;
  if (!d_s || !d_a || !d_lp || !d_v) {
    const size_t f = sizeof(float) * n;
    if (carve(c, &c->scratch, &c->scratch_bytes, {{&r_s, 12 * f}, {&r_a, 4 * f}, {&r_lp, 4 * f}, {&r_v, f}}))
      return WK_ERR_HIP;
  }
  for (int j = 0; j < k; j++) {
    float* s_row = d_s ? d_s + 12 * n * j : r_s;
    float* a_row = d_a ? d_a + 4 * n * j : r_a;
    HIPCHK(c, wk::launch_get_obs(c->P, c->st, s_row, c->stream));
    HIPCHK(c, launch_policy_for(c, c->n, s_row, nullptr, c->rng_t, nullptr, a_row,
                                d_lp ? d_lp + 4 * n * j : r_lp, d_v ? d_v + n * j : r_v));
    wk::StepArgs A = env_args(c);
    A.actions = a_row;
    A.obs_out = d_obs ? d_obs + 12 * n * j : nullptr;
    A.pos_out = d_pos ? d_pos + 2 * n * j : nullptr;
    A.rew_out = d_r ? d_r + n * j : nullptr;
    A.done_out = d_d ? d_d + n * j : nullptr;
    A.fault_out = d_fault;
    A.k_steps = 1;
    HIPCHK(c, launch_physics(c, 0, A));
  }
  return WK_OK;
}

// A.k_steps sampled env-steps recorded into A's rows: the fused kernel, or net_sampled
int sampled_steps(wk_ctx* c, wk::StepArgs& A) {
  ProfScope ps(c, PK_PHYS, (int64_t)A.k_steps * c->n);
  if (c->general)
    return net_sampled(c, A.k_steps, A.traj_s, A.traj_a, A.traj_lp, A.traj_v, A.traj_r, A.traj_d, A.obs_out,
                       A.pos_out, A.fault_out);
  HIPCHK(c, launch_physics(c, 3, A));
  return WK_OK;
}

static int step_impl(wk_ctx* c, const float* d_actions, int k, float* d_obs, float* d_rew,
                     uint8_t* d_done, uint32_t* d_fault, int mode, void* trace) {
  if (c->general && mode >= 2) {
    ProfScope ps(c, PK_PHYS, (int64_t)k * c->n);
    return net_sampled(c, k, nullptr, nullptr, nullptr, nullptr, d_rew, d_done, d_obs, nullptr, d_fault);
  }
  wk::StepArgs A = policy_args(c);
  A.actions = d_actions; A.obs_out = d_obs; A.rew_out = d_rew; A.done_out = d_done;
  A.fault_out = d_fault;
  A.trace = (wk::PairTraceDev*)trace;
  A.k_steps = k;
  ProfScope ps(c, PK_PHYS, (int64_t)k * c->n);
  HIPCHK(c, launch_physics(c, mode, A));
  return WK_OK;
}

int wk_step_device(wk_ctx* c, const float* d_actions, int k, float* d_obs, float* d_rew,
                   uint8_t* d_done, uint32_t* d_fault) {
  DevGuard dg_(c);
  if (!c || k <= 0) return WK_ERR_ARG;
  return step_impl(c, d_actions, k, d_obs, d_rew, d_done, d_fault, d_actions ? 0 : 2, nullptr);
}

int wk_step(wk_ctx* c, const float* actions, int k, float* obs, float* reward, uint8_t* done,
            uint32_t* fault) {
  DevGuard dg_(c);
  if (!c || k <= 0) return WK_ERR_ARG;
  const size_t n = c->n;
  const size_t b_act = actions ? sizeof(float) * 4 * n * k : 0;
  const size_t b_obs = sizeof(float) * 12 * n * k, b_rew = sizeof(float) * n * k, b_done = n * k;
  const size_t b_fault = sizeof(uint32_t) * n;
  float *d_act, *d_obs, *d_rew;  // (d_act null without actions: no bytes)
  uint32_t* d_fault;
  uint8_t* d_done;
  if (carve(c, &c->scratch2, &c->scratch2_bytes,
            {{&d_act, b_act}, {&d_obs, b_obs}, {&d_rew, b_rew}, {&d_fault, b_fault}, {&d_done, b_done}}))
    return WK_ERR_HIP;
  if (actions) HIPCHK(c, hipMemcpyAsync(d_act, actions, b_act, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_fault, 0, b_fault, c->stream));
  int r = step_impl(c, d_act, k, obs ? d_obs : nullptr, reward ? d_rew : nullptr,
                    done ? d_done : nullptr, d_fault, actions ? 0 : 2, nullptr);
  if (r) return r;
  if (obs) HIPCHK(c, hipMemcpyAsync(obs, d_obs, b_obs, hipMemcpyDeviceToHost, c->stream));
  if (reward) HIPCHK(c, hipMemcpyAsync(reward, d_rew, b_rew, hipMemcpyDeviceToHost, c->stream));
  if (done) HIPCHK(c, hipMemcpyAsync(done, d_done, b_done, hipMemcpyDeviceToHost, c->stream));
  if (fault) HIPCHK(c, hipMemcpyAsync(fault, d_fault, b_fault, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

// ---------------- the reference's per-body call shape ----------------
// Environment.StepObjects (Environment.cs:126-143) calls, per substep, Joint.Step on the 4 joints
// and IObject.Update (Objects/IObject.cs:9) on every body of the list: list_count * Iterations
// Update calls per frame.  The GPU resolves the whole frame in one launch, so the frame's FIRST
// Update call runs one env-step of every walker and the rest are counted no-ops; the torques are
// the ones Walker.TakeActions (Walker.cs:66-75) stored since the last frame, and a walker given
// none keeps its joints' current torques (Joint.SetTorque with the same value: no kick,
// Joint.cs:56-61) -- as in the reference, where nothing else changes them.
static int current_torques(wk_ctx* c, float* out /* [n][4] */) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy2D(out, sizeof(float) * 4, c->st + wk::S_TORQUE, sizeof(float) * wk::NSTATE,
                        sizeof(float) * 4, c->n, hipMemcpyDeviceToHost));
  return WK_OK;
}

int wk_take_actions(wk_ctx* c, int env, const float* actions) {
  if (!c || !actions || env < 0 || env >= c->n) return WK_ERR_ARG;
  if (c->pend_set.empty()) {
    c->pend.assign((size_t)c->n * 4, 0.0f);
    c->pend_set.assign((size_t)c->n, 0);
  }
  for (int j = 0; j < 4; j++) c->pend[(size_t)env * 4 + j] = actions[j];
  c->pend_set[env] = 1;
  return WK_OK;
}

int wk_object_update(wk_ctx* c, int list_count, float delta_time) {
  DevGuard dg_(c);
  if (!c || list_count <= 0 || !(delta_time >= 0.0f)) return WK_ERR_ARG;
  int stepped = 0;
  if (c->frame_calls == 0) {
    c->frame_len = (int64_t)list_count * c->cfg.Iterations;
    std::vector<float> a((size_t)c->n * 4);
    if (int r = current_torques(c, a.data())) return r;  // (the state as of this frame)
    for (size_t e = 0; e < c->pend_set.size(); e++)
      if (c->pend_set[e])
        for (int j = 0; j < 4; j++) a[e * 4 + j] = c->pend[e * 4 + j];
    std::fill(c->pend_set.begin(), c->pend_set.end(), (uint8_t)0);
    if (int r = wk_step(c, a.data(), 1, nullptr, nullptr, nullptr, nullptr)) return r;
    stepped = 1;
  }
  if (++c->frame_calls >= c->frame_len) c->frame_calls = 0;
  return stepped;
}

int wk_joint_step(wk_ctx* c) { return c ? WK_OK : WK_ERR_ARG; }

int wk_body_order(wk_ctx* c, int env, int* parts, int* count) {
  DevGuard dg_(c);
  if (!c || !parts || !count || env < 0 || env >= c->n) return WK_ERR_ARG;
  float post = 0.0f;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&post, c->st + (size_t)env * wk::NSTATE + wk::S_POSTRESET, sizeof(float),
                      hipMemcpyDeviceToHost));
  const int nfloor = c->P.rough ? 10 : 1;  // the floor body ids are 5 .. 5 + nfloor - 1
  int k = 0;
  if (post != 0.0f)
    for (int f = 0; f < nfloor; f++) parts[k++] = 5 + f;
  for (int b = 0; b < 5; b++) parts[k++] = b;  // CreateBodies' order: LLL, LLU, Body, RLL, RLU
  if (post == 0.0f)
    for (int f = 0; f < nfloor; f++) parts[k++] = 5 + f;
  *count = k;
  return WK_OK;
}

int wk_step_sampled(wk_ctx* c, int k, float* states, float* actions, float* logp, float* values,
                    float* reward, uint8_t* done, float* next_obs, uint32_t* fault,
                    float* position) {
  DevGuard dg_(c);
  if (!c || k <= 0) return WK_ERR_ARG;
  const size_t n = c->n, kn = (size_t)k * n;
  // the policy-sampling kernel with RECORD rows pointed at scratch (the device trajectory
  // buffer of wk_rollout is not touched)
  const size_t b12 = sizeof(float) * 12 * kn, b4 = sizeof(float) * 4 * kn, b1 = sizeof(float) * kn;
  const size_t b_fault = sizeof(uint32_t) * n;
  const size_t b_pos = sizeof(float) * 2 * kn;
  float *d_s, *d_a, *d_lp, *d_v, *d_r, *d_o, *d_pos;
  uint32_t* d_f;
  uint8_t* d_d;
  if (carve(c, &c->scratch2, &c->scratch2_bytes,
            {{&d_s, b12}, {&d_a, b4}, {&d_lp, b4}, {&d_v, b1}, {&d_r, b1}, {&d_o, b12}, {&d_f, b_fault},
             {&d_pos, b_pos}, {&d_d, kn}}))
    return WK_ERR_HIP;
  HIPCHK(c, hipMemsetAsync(d_f, 0, b_fault, c->stream));
  wk::StepArgs A = policy_args(c);
  set_traj(A, d_s, d_a, d_lp, d_r, d_d, d_v);
  A.obs_out = next_obs ? d_o : nullptr; A.fault_out = d_f;
  A.pos_out = position ? d_pos : nullptr;
  A.k_steps = k;
  if (int r = sampled_steps(c, A)) return r;
  if (states) HIPCHK(c, hipMemcpyAsync(states, d_s, b12, hipMemcpyDeviceToHost, c->stream));
  if (actions) HIPCHK(c, hipMemcpyAsync(actions, d_a, b4, hipMemcpyDeviceToHost, c->stream));
  if (logp) HIPCHK(c, hipMemcpyAsync(logp, d_lp, b4, hipMemcpyDeviceToHost, c->stream));
  if (values) HIPCHK(c, hipMemcpyAsync(values, d_v, b1, hipMemcpyDeviceToHost, c->stream));
  if (reward) HIPCHK(c, hipMemcpyAsync(reward, d_r, b1, hipMemcpyDeviceToHost, c->stream));
  if (done) HIPCHK(c, hipMemcpyAsync(done, d_d, kn, hipMemcpyDeviceToHost, c->stream));
  if (next_obs) HIPCHK(c, hipMemcpyAsync(next_obs, d_o, b12, hipMemcpyDeviceToHost, c->stream));
  if (fault) HIPCHK(c, hipMemcpyAsync(fault, d_f, b_fault, hipMemcpyDeviceToHost, c->stream));
  if (position) HIPCHK(c, hipMemcpyAsync(position, d_pos, b_pos, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_step_traced(wk_ctx* c, const float* actions, wk_pair_trace* trace) {
  DevGuard dg_(c);
  if (!c || !actions || !trace) return WK_ERR_ARG;
  static_assert(sizeof(wk_pair_trace) == sizeof(wk::PairTraceDev), "trace layout");
  const size_t n = c->n;
  const size_t b_act = sizeof(float) * 4 * n;
  const size_t b_tr = sizeof(wk_pair_trace) * n * c->cfg.Iterations;
  float* d_act;
  void* d_tr;
  if (carve(c, &c->scratch2, &c->scratch2_bytes, {{&d_act, b_act}, {&d_tr, b_tr}})) return WK_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d_act, actions, b_act, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_tr, 0, b_tr, c->stream));
  int r = step_impl(c, d_act, 1, nullptr, nullptr, nullptr, nullptr, 1, d_tr);
  if (r) return r;
  HIPCHK(c, hipMemcpyAsync(trace, d_tr, b_tr, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_get_obs(wk_ctx* c, float* obs) {
  DevGuard dg_(c);
  if (!c || !obs) return WK_ERR_ARG;
  if (ensure(c, &c->scratch, &c->scratch_bytes, sizeof(float) * 12 * c->n)) return WK_ERR_HIP;
  HIPCHK(c, wk::launch_get_obs(c->P, c->st, (float*)c->scratch, c->stream));
  HIPCHK(c, hipMemcpyAsync(obs, c->scratch, sizeof(float) * 12 * c->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

// the device state is [n_env][WK_STATE_FLOATS] (one 448-B record per walker), the same
// layout as the canonical dump, so these are plain copies
int wk_get_state(wk_ctx* c, float* state) {
  DevGuard dg_(c);
  if (!c || !state) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(state, c->st, sizeof(float) * wk::NSTATE * c->n, hipMemcpyDeviceToHost));
  return WK_OK;
}

// the rigid-pole shortcut (pole_own_minmax, csrc/wk_device.h) projects a walker
// pole onto its own edge axes with min / max over fixed vertex groups, which equals the reference's
// min / max over all six vertices (SATCollision.cs:63-76 ProjectPoints) only while the pole keeps
// its template shape (Pole.FromSize, Pole.cs:18-34): every vertex left out of a group lies >= 7.5
// px beyond the group's extreme.  A state from outside (wk_set_state, wk_checkpoint_load) must keep
// that margin; the kernel's own states do (rigid motion, << 1 px of rounding drift).
// Required margin: POLE_MARGIN_PX, above the worst-case drift bound (~3 px over 50,000 substeps).
// Poles with a non-finite coordinate are not checked (the NaN path is exact).
static constexpr double POLE_MARGIN_PX = 3.5;
static const int kPoleGroups[6][2][3] = {  // per own edge: {min group, max group}, -1 = unused
    {{0, 1, 2}, {3, 4, 5}}, {{0, 1, 2}, {3, 4, 5}}, {{2, 3, -1}, {5, 0, -1}},
    {{3, 4, 5}, {0, 1, 2}}, {{3, 4, 5}, {0, 1, 2}}, {{5, 0, -1}, {2, 3, -1}}};
// the smallest margin of one pole (record floats x0 y0 .. x5 y5), or +inf if non-finite
static double pole_margin(const float* v) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(v[i])) return INFINITY;
  double worst = INFINITY;
  for (int e = 0; e < 6; e++) {
    const int e1 = (e + 1) % 6;
    const double ex = (double)v[2 * e1] - v[2 * e], ey = (double)v[2 * e1 + 1] - v[2 * e + 1];
    const double len = std::sqrt(ex * ex + ey * ey);
    if (!(len > 0.0)) return -INFINITY;  // a zero edge: not a rigid template pole
    const double ax = -ey / len, ay = ex / len;
    double p[6];
    for (int i = 0; i < 6; i++) p[i] = ax * v[2 * i] + ay * v[2 * i + 1];
    bool inmin[6] = {}, inmax[6] = {};
    double gmin = INFINITY, gmax = -INFINITY;
    for (int k = 0; k < 3; k++) {
      const int a = kPoleGroups[e][0][k], b = kPoleGroups[e][1][k];
      if (a >= 0) { inmin[a] = true; gmin = std::min(gmin, p[a]); }
      if (b >= 0) { inmax[b] = true; gmax = std::max(gmax, p[b]); }
    }
    for (int i = 0; i < 6; i++) {
      if (!inmin[i]) worst = std::min(worst, p[i] - gmin);
      if (!inmax[i]) worst = std::min(worst, gmax - p[i]);
    }
  }
  return worst;
}

int wk_check_state(const float* state, int n_env, int* bad_env, int* bad_body) {
  if (!state || n_env <= 0) return WK_ERR_ARG;
  static const int poles[4] = {wk::LLL, wk::LLU, wk::RLL, wk::RLU};
  for (int e = 0; e < n_env; e++)
    for (int b : poles)
      if (!(pole_margin(state + (size_t)e * wk::NSTATE + (size_t)b * wk::BSTRIDE) >= POLE_MARGIN_PX)) {
        if (bad_env) *bad_env = e;
        if (bad_body) *bad_body = b;
        return WK_ERR_ARG;
      }
  if (bad_env) *bad_env = -1;
  if (bad_body) *bad_body = -1;
  return WK_OK;
}

int check_state_or_fail(wk_ctx* c, const float* state) {
  int e = -1, b = -1;
  if (wk_check_state(state, c->n, &e, &b) != WK_OK) {
    SETERR(c, "walker %d body %d is not a rigid walker pole (a vertex group closer than %.1f px to "
           "the excluded vertices on one of its own edge axes: deformed or reordered vertices); "
           "the state is refused", e, b, POLE_MARGIN_PX);
    return WK_ERR_ARG;
  }
  return WK_OK;
}

int wk_set_state(wk_ctx* c, const float* state) {
  DevGuard dg_(c);
  if (!c || !state) return WK_ERR_ARG;
  if (int r = check_state_or_fail(c, state)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->st, state, sizeof(float) * wk::NSTATE * c->n, hipMemcpyHostToDevice));
  return WK_OK;
}

int wk_get_body_view(wk_ctx* c, int env, int body, wk_body_view* o) {
  DevGuard dg_(c);
  if (!c || !o || env < 0 || env >= c->n || body < 0 || body >= (c->P.rough ? 15 : 6)) return WK_ERR_ARG;
  memset(o, 0, sizeof(*o));
  if (c->P.rough && body >= 5) {  // rough-floor segment body - 5 (Environment.cs:230-261)
    const int k = body - 5;
    const uint32_t gid = (uint32_t)(c->cfg.EnvOffset + env);
    const float x = -50.0f + 120.0f * (float)k;
    const float yp = 800.0f + (float)wk::terrain_draw(c->seed, gid, k);
    const float y = 800.0f + (float)wk::terrain_draw(c->seed, gid, k + 1);
    const float v[4][2] = {{x, 1050.0f}, {k == 0 ? x : x - 120.0f, yp}, {x, y}, {x + 120.0f, 1050.0f}};
    float sx = 0.0f, sy = 0.0f;
    o->n_vertices = 4;
    for (int i = 0; i < 4; i++) {
      o->vertices[i][0] = v[i][0]; o->vertices[i][1] = v[i][1];
      sx += v[i][0]; sy += v[i][1];
    }
    o->centroid[0] = sx * 0.25f; o->centroid[1] = sy * 0.25f;  // FindCentroid: sum * (1/4)
    o->is_static = 1;
    return WK_OK;
  }
  if (body == 5) {  // the static Metal floor (Environment.cs:219-223)
    const float fl[4][2] = {{-50, 1050}, {-50, 900}, {1050, 900}, {1050, 1050}};
    o->n_vertices = 4;
    for (int i = 0; i < 4; i++) { o->vertices[i][0] = fl[i][0]; o->vertices[i][1] = fl[i][1]; }
    o->centroid[0] = 500.0f; o->centroid[1] = 975.0f;
    o->is_static = 1;
    return WK_OK;
  }
  float f[wk::BSTRIDE];
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(f, c->st + (size_t)env * wk::NSTATE + (size_t)body * wk::BSTRIDE,
                      sizeof(f), hipMemcpyDeviceToHost));
  o->n_vertices = body == wk::BODY ? 5 : 6;
  for (int i = 0; i < o->n_vertices; i++) { o->vertices[i][0] = f[2 * i]; o->vertices[i][1] = f[2 * i + 1]; }
  o->centroid[0] = f[wk::F_CX]; o->centroid[1] = f[wk::F_CY];
  o->linear_velocity[0] = f[wk::F_VX]; o->linear_velocity[1] = f[wk::F_VY];
  o->angular_velocity = f[wk::F_W];
  o->angle = f[wk::F_TH];
  o->collided = f[wk::F_COL] != 0.0f;
  return WK_OK;
}

// ---------------- scene props (wk_env_scene.h) ----------------
// <Shape>.FromSize (Square.cs:18-31, Triangle.cs:18-30, Hexagon.cs:18-33) then
// Skeleton.SmoothCorners (Skeleton.cs:33-53) in host fp32 (built with -ffp-contract=off,
// the same IEEE ops as the oracle); returns the vertex count or -1
int prop_vertices(const wk_prop& p, int smooth, float* xs, float* ys) {
  const float cx = p.cx, cy = p.cy, adj = (float)0.5 * p.size;
  int n;
  if (p.shape == WK_SHAPE_SQUARE) {
    const float vx[4] = {cx + adj, cx - adj, cx - adj, cx + adj};
    const float vy[4] = {cy + adj, cy + adj, cy - adj, cy - adj};
    n = 4;
    for (int i = 0; i < n; i++) { xs[i] = vx[i]; ys[i] = vy[i]; }
  } else if (p.shape == WK_SHAPE_TRIANGLE) {
    const float vx[3] = {cx, cx - adj, cx + adj};
    const float vy[3] = {cy + adj, cy - adj, cy - adj};
    n = 3;
    for (int i = 0; i < n; i++) { xs[i] = vx[i]; ys[i] = vy[i]; }
  } else if (p.shape == WK_SHAPE_HEXAGON) {
    const float h = adj * 0.5f;
    const float vx[6] = {cx + h, cx - h, cx - adj, cx - h, cx + h, cx + adj};
    const float vy[6] = {cy + adj, cy + adj, cy, cy - adj, cy - adj, cy};
    n = 6;
    for (int i = 0; i < n; i++) { xs[i] = vx[i]; ys[i] = vy[i]; }
  } else {
    return -1;
  }
  for (int it = 0; it < smooth; it++) {
    if (2 * n > WK_PROP_MAXV) return -1;
    float nx[WK_PROP_MAXV], ny[WK_PROP_MAXV];
    for (int j = 0; j < n; j++) {
      const int a = (j + 1) % n, b = (j + n - 1) % n;  // ContactPoints.Mod(j - 1, n)
      const float abx = (xs[a] - xs[j]) * 0.2f, aby = (ys[a] - ys[j]) * 0.2f;
      const float acx = (xs[b] - xs[j]) * 0.2f, acy = (ys[b] - ys[j]) * 0.2f;
      nx[2 * j] = xs[j] + acx; ny[2 * j] = ys[j] + acy;
      nx[2 * j + 1] = xs[j] + abx; ny[2 * j + 1] = ys[j] + aby;
    }
    n *= 2;
    for (int i = 0; i < n; i++) { xs[i] = nx[i]; ys[i] = ny[i]; }
  }
  return n;
}

static const float kMatProps[8][3] = {  // Materials/*.cs: inverse mass, restitution, friction
    {5.0f, 0.3f, 0.8f}, {11.0f, 0.3f, 0.0f}, {11.0f, 0.7f, 0.5f}, {15.0f, 0.3f, 1.0f},
    {20.0f, 0.3f, 0.01f}, {1.0f, 0.3f, 0.1f}, {0.01f, 0.1f, 0.2f}, {11.0f, 1.0f, 1.0f}};

int wk_set_scene(wk_ctx* c, const wk_prop* props, int n_props) {
  DevGuard dg_(c);
  if (!c || n_props < 0 || (n_props > 0 && !props)) return WK_ERR_ARG;
  if (n_props > WK_MAX_PROPS) { SETERR(c, "at most %d scene props", (int)WK_MAX_PROPS); return WK_ERR_ARG; }
  if (n_props > 0 && c->cfg.LanesPerWalker > 1) {
    SETERR(c, "scene props run on the one-lane mapping (LanesPerWalker 0 or 1)");
    return WK_ERR_CONFIG;
  }
  wk::SceneDev S{};
  std::vector<float> rec;
  for (int k = 0; k < n_props; k++) {
    const wk_prop& p = props[k];
    const float fin[8] = {p.cx, p.cy, p.size, p.vx, p.vy, p.w, p.ax, p.ay};
    for (float f : fin)
      if (!std::isfinite(f)) { SETERR(c, "prop %d: non-finite parameter", k); return WK_ERR_ARG; }
    if (p.material < 0 || p.material > 7 || p.smooth < 0 || !(p.size > 0.0f)) {
      SETERR(c, "prop %d: invalid material, smooth count or size", k);
      return WK_ERR_ARG;
    }
    float xs[WK_PROP_MAXV], ys[WK_PROP_MAXV], bx[WK_PROP_MAXV], by[WK_PROP_MAXV];
    const int nv = prop_vertices(p, p.smooth, xs, ys);
    if (nv < 0) { SETERR(c, "prop %d: unknown shape or more than %d vertices", k, (int)WK_PROP_MAXV); return WK_ERR_ARG; }
    if ((int)rec.size() + 2 * nv + 6 > wk::SCENE_FIELDS) {
      SETERR(c, "scene props exceed %d vertices in total", (int)WK_SCENE_MAX_VERTS);
      return WK_ERR_ARG;
    }
    int total = nv;
    for (int j = 0; j < k; j++) total += S.nv[j];
    if (total > WK_SCENE_MAX_VERTS) { SETERR(c, "scene props exceed %d vertices in total", (int)WK_SCENE_MAX_VERTS); return WK_ERR_ARG; }
    // Skeleton.AddVectors -> FindCentroid of the FromSize vertices (before SmoothCorners)
    const int nb = prop_vertices(p, 0, bx, by);
    float sx = 0.0f, sy = 0.0f;
    for (int i = 0; i < nb; i++) { sx = sx + bx[i]; sy = sy + by[i]; }
    const float inv = 1.0f / (float)nb;
    S.nv[k] = nv;
    S.off[k] = (int)rec.size();
    S.stat[k] = p.is_static ? 1 : 0;
    // RigidBody ctor (RigidBody.cs:36-50)
    S.im[k] = p.is_static ? 0.0f : kMatProps[p.material][0];
    S.ii[k] = p.is_static ? 0.0f : 0.001f * kMatProps[p.material][0];
    S.e[k] = kMatProps[p.material][1];
    S.mu[k] = kMatProps[p.material][2];
    S.adx[k] = p.ax * c->P.dt_sub;  // _acceleration * deltaTime (StepLinearVelocity)
    S.ady[k] = p.ay * c->P.dt_sub;
    for (int i = 0; i < nv; i++) rec.push_back(xs[i]);
    for (int i = 0; i < nv; i++) rec.push_back(ys[i]);
    const float tail[6] = {sx * inv, sy * inv, p.vx, p.vy, p.w, 0.0f};
    for (float f : tail) rec.push_back(f);
  }
  S.n_props = n_props;
  S.pstride = (int)rec.size();
  // the new block is the context's from its allocation on: no path below has to free it
  if (c->props_next) (void)hipFree(c->props_next);
  c->props_next = nullptr;
  if (n_props > 0) {
    std::vector<float> all((size_t)c->n * rec.size());
    for (int e = 0; e < c->n; e++) memcpy(all.data() + (size_t)e * rec.size(), rec.data(), sizeof(float) * rec.size());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, dev_alloc(c, &c->props_next, sizeof(float) * all.size()));
    if (hipMemcpy(c->props_next, all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice) != hipSuccess) {
      SETERR(c, "scene upload failed");
      return WK_ERR_HIP;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->props) (void)hipFree(c->props);
  c->props = c->props_next;
  c->props_next = nullptr;
  c->scene = S;
  c->snap_valid = false;  // the snapshot's layout no longer matches
  c->scene_desc.assign(props, props + n_props);
  return WK_OK;
}

int wk_get_prop_view(wk_ctx* c, int env, int k, wk_prop_view* o) {
  DevGuard dg_(c);
  if (!c || !o || env < 0 || env >= c->n || k < 0 || k >= c->scene.n_props) return WK_ERR_ARG;
  memset(o, 0, sizeof(*o));
  const int nv = c->scene.nv[k];
  std::vector<float> f(2 * nv + 6);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(f.data(), c->props + (size_t)env * c->scene.pstride + c->scene.off[k],
                      sizeof(float) * f.size(), hipMemcpyDeviceToHost));
  o->n_vertices = nv;
  for (int i = 0; i < nv; i++) { o->vertices[i][0] = f[i]; o->vertices[i][1] = f[nv + i]; }
  o->centroid[0] = f[2 * nv]; o->centroid[1] = f[2 * nv + 1];
  o->linear_velocity[0] = f[2 * nv + 2]; o->linear_velocity[1] = f[2 * nv + 3];
  o->angular_velocity = f[2 * nv + 4];
  o->angle = f[2 * nv + 5];
  o->is_static = c->scene.stat[k];
  return WK_OK;
}

int wk_rollout_mapping(wk_ctx* c, int* lanes_per_walker, int* walkers_per_wave, int64_t* waves,
                       int64_t* waves_launched) {
  if (!c || !lanes_per_walker || !walkers_per_wave || !waves) return WK_ERR_ARG;
  const int64_t n = c->n;
  int64_t launched;
  if (c->scene.n_props > 0) {  // the one-lane scene kernel (64-thread blocks)
    *lanes_per_walker = 1; *walkers_per_wave = 64; *waves = (n + 63) / 64;
    launched = *waves;
  } else {
    const int L = c->P.lanes;
    *lanes_per_walker = L;
    if (L == 4) {  // sparse quad: wpw walkers in the first 4 wpw lanes of each wave
      *walkers_per_wave = c->P.wpw;
      *waves = (n + c->P.wpw - 1) / c->P.wpw;
    } else {
      *walkers_per_wave = 64 / L;
      *waves = (n * L + 63) / 64;
    }
    launched = *waves;
    if (L == 2 || L == 4) {  // k_env_side launches whole SIDE_BLOCK blocks: the idle
      // waves of the last block still run the loop, replaying the last walker
      constexpr int64_t wpb = wk::SIDE_BLOCK_THREADS / 64;
      launched = (*waves + wpb - 1) / wpb * wpb;
    }
  }
  if (waves_launched) *waves_launched = launched;
  return WK_OK;
}

int wk_count_events(wk_ctx* c, int k, uint64_t* counts) {
  DevGuard dg_(c);
  if (!c || !counts || k <= 0) return WK_ERR_ARG;
  if (k > c->T_valid) { SETERR(c, "count replay of %d env-steps, the trajectory holds %d", k, c->T_valid); return WK_ERR_STATE; }
  if (c->scene.n_props > 0) { SETERR(c, "the counting replay runs without scene props"); return WK_ERR_CONFIG; }
  static_assert(WK_NEV == wk::NEV, "event counters");
  if (!c->counts) HIPCHK(c, dev_alloc(c, &c->counts, sizeof(unsigned long long) * wk::NEV));
  HIPCHK(c, hipMemsetAsync(c->counts, 0, sizeof(unsigned long long) * wk::NEV, c->stream));
  wk::StepArgs A = env_args(c);
  A.actions = c->ta; A.k_steps = k; A.counts = c->counts;
  HIPCHK(c, wk::launch_env_step(4, c->P, A, c->stream));
  unsigned long long h[wk::NEV];
  HIPCHK(c, hipMemcpyAsync(h, c->counts, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < wk::NEV; i++) counts[i] += (uint64_t)h[i];
  return WK_OK;
}
