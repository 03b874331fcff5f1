// wk_api_rollout.cpp -- collecting a trajectory: wk_policy_sample / wk_value, wk_rollout with its
// bootstrap values and returns, the trajectory's get / set, reward normalisation, and the data
// collection (episode and loss logs, the data file).
#include <cmath>
#include <cstring>

#include "wk_ctx.h"
#include "wk_text.h"

static int policy_impl(wk_ctx* c, int n, const float* obs, const int32_t* ids, const uint32_t* steps,
                       float* mean, float* act, float* logp, float* v) {
  const size_t b_obs = sizeof(float) * 12 * n, b4 = sizeof(float) * 4 * n, b1 = sizeof(float) * n;
  float *d_obs, *d_mean, *d_act, *d_lp, *d_v;
  int32_t* d_ids;
  uint32_t* d_steps;
  if (carve(c, &c->scratch2, &c->scratch2_bytes,
            {{&d_obs, b_obs}, {&d_mean, b4}, {&d_act, b4}, {&d_lp, b4}, {&d_v, b1},
             {&d_ids, sizeof(int32_t) * n}, {&d_steps, sizeof(uint32_t) * n}}))
    return WK_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d_obs, obs, b_obs, hipMemcpyHostToDevice, c->stream));
  if (ids) HIPCHK(c, hipMemcpyAsync(d_ids, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
  if (steps) HIPCHK(c, hipMemcpyAsync(d_steps, steps, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_policy_for(c, n, d_obs, ids ? d_ids : nullptr, steps ? d_steps : nullptr,
                              v ? nullptr : d_mean, v ? nullptr : d_act, v ? nullptr : d_lp,
                              v ? d_v : nullptr));
  // (wk_value passes v alone, wk_policy_sample the other three)
  if (v) HIPCHK(c, hipMemcpyAsync(v, d_v, b1, hipMemcpyDeviceToHost, c->stream));
  if (mean) HIPCHK(c, hipMemcpyAsync(mean, d_mean, b4, hipMemcpyDeviceToHost, c->stream));
  if (act) HIPCHK(c, hipMemcpyAsync(act, d_act, b4, hipMemcpyDeviceToHost, c->stream));
  if (logp) HIPCHK(c, hipMemcpyAsync(logp, d_lp, b4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_policy_sample(wk_ctx* c, int n, const float* obs, const int32_t* env_ids,
                     const uint32_t* steps, float* mean, float* act, float* logp) {
  DevGuard dg_(c);
  if (!c || n <= 0 || !obs) return WK_ERR_ARG;
  return policy_impl(c, n, obs, env_ids, steps, mean, act, logp, nullptr);
}

int wk_value(wk_ctx* c, int n, const float* obs, float* v) {
  DevGuard dg_(c);
  if (!c || n <= 0 || !obs || !v) return WK_ERR_ARG;
  return policy_impl(c, n, obs, nullptr, nullptr, nullptr, nullptr, nullptr, v);
}

// ReturnsMode = 1: the critic's value of every walker's current observation (post-reset after a
// terminal step) into vlast, with the kernels of wk_value -- bit-equal to wk_value(wk_get_obs())
static int bootstrap_values(wk_ctx* c) {
  if (ensure(c, &c->scratch, &c->scratch_bytes, sizeof(float) * 12 * c->n)) return WK_ERR_HIP;
  float* obs = (float*)c->scratch;
  ProfScope ps(c, PK_RET);
  HIPCHK(c, wk::launch_get_obs(c->P, c->st, obs, c->stream));
  HIPCHK(c, launch_policy_for(c, c->n, obs, nullptr, nullptr, nullptr, nullptr, nullptr, c->vlast));
  c->vlast_valid = true;
  return WK_OK;
}

// Reward normalisation over the valid trajectory buffer (wk_rnorm.hip), timed in the returns slot.
// learn: the full pass -- the scan carries rn_acc, the finish step merges the batch into rn_rec and
// forms the scale, the apply step writes trs; otherwise, and on a frozen context, the apply step
// alone with the scale as it is.
// On a record-exchange context the full pass is collective: scan and this rank's batch record, the
// gather of the ranks' records (RCCL: on the stream, no wait; host: through the callback), then the
// rank-ordered fold, the merge and the apply step -- the same statistics bytes on every rank.
static int rnorm_pass(wk_ctx* c, bool learn) {
  ProfScope ps(c, PK_RET);
  if (learn && !c->rn_frozen && records_on(c)) {
    const uint64_t header = rx_header(c, 2);
    HIPCHK(c, wk::launch_rnorm_batch(c->n, c->T_valid, c->cfg.Gamma, c->tr, c->td, c->rn_acc, c->rn_partial,
                                     header, c->rx_dev + (size_t)c->rank * wk::RECORD_WORDS, c->stream));
    if (int r = rx_gather_device(c, header)) return r;
    HIPCHK(c, wk::launch_rnorm_merge(c->n, c->T_valid, c->rn_clip, c->rn_eps, c->rx_dev, c->nranks, header,
                                     c->rx_err, c->tr, c->rn_rec, c->trs, c->stream));
    return WK_OK;
  }
  HIPCHK(c, wk::launch_rnorm_pass(c->n, c->T_valid, c->cfg.Gamma, c->rn_clip, c->rn_eps,
                                  learn && !c->rn_frozen, c->tr, c->td, c->rn_acc, c->rn_partial,
                                  c->rn_rec, c->trs, c->stream));
  return WK_OK;
}

int returns_impl(wk_ctx* c) {
  if (c->cfg.ReturnsMode == 1 && !c->vlast_valid) {
    SETERR(c, "ReturnsMode 1: the trajectory has no bootstrap values -- call wk_set_bootstrap_values "
              "(zeros for complete episodes, wk_value of the next observations at a cut)");
    return WK_ERR_STATE;
  }
  const float* rew = c->rn_on ? c->trs : c->tr;  // (reward normalisation: the scaled rewards)
  {
    ProfScope ps(c, PK_RET);
    HIPCHK(c, wk::launch_returns(c->cfg.ReturnsMode, c->n, c->T_valid, c->cfg.UseGAE, c->cfg.Gamma,
                                 c->cfg.Lambda, rew, c->tv, c->td, c->vlast, c->tret, c->tadv, c->stream));
  }
  if (c->cfg.NormalizeAdvantages)
    HIPCHK(c, wk::launch_normalize(c->tadv, c->n * c->T_valid, c->cfg.Epsilon, c->stream));
  c->returns_valid = true;
  return WK_OK;
}

int wk_rollout(wk_ctx* c, int horizon) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (horizon <= 0) horizon = c->T;
  if (horizon > c->T) { SETERR(c, "horizon %d exceeds the configured Horizon %d", horizon, c->T); return WK_ERR_ARG; }
  wk::StepArgs A = policy_args(c);
  A.k_steps = horizon;
  if (int r = sampled_steps(c, A)) return r;
  c->T_valid = horizon;
  if (c->collect) {
    wk::EpisodeArgs e{c->n, horizon, c->cfg.EnvOffset, c->rollout_steps, c->tr, c->td, c->ep_acc,
                      c->ep_len, (float2*)c->ep_scratch, c->ep_rowcnt, c->ep_count, c->ep_cap,
                      c->ep_log};
    ProfScope ps(c, PK_RET);
    HIPCHK(c, wk::launch_episode_log(e, c->stream));
  }
  c->rollout_steps += (uint32_t)horizon;
  if (c->rn_on)
    if (int r = rnorm_pass(c, true)) return r;
  if (c->cfg.ReturnsMode == 1)
    if (int r = bootstrap_values(c)) return r;
  return returns_impl(c);
}

int wk_compute_returns(wk_ctx* c) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (c->T_valid <= 0) { SETERR(c, "no trajectory recorded"); return WK_ERR_STATE; }
  return returns_impl(c);
}

int wk_rollout_stats_get(wk_ctx* c, wk_rollout_stats* o) {
  DevGuard dg_(c);
  if (!c || !o) return WK_ERR_ARG;
  memset(o, 0, sizeof(*o));
  const size_t cnt = (size_t)c->n * c->T_valid;
  std::vector<float> r(cnt);
  std::vector<uint8_t> d(cnt);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (cnt) {
    HIPCHK(c, hipMemcpy(r.data(), c->tr, sizeof(float) * cnt, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d.data(), c->td, cnt, hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < cnt; i++) { o->reward_sum += r[i]; o->episodes += d[i]; }
  o->env_steps = (int64_t)cnt;
  return WK_OK;
}

int wk_get_trajectory(wk_ctx* c, float* s, float* a, float* lp, float* r, uint8_t* d, float* v,
                      float* ret, float* adv) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  const size_t cnt = (size_t)c->n * c->T_valid;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  void* const host[8] = {s, a, lp, r, d, v, ret, adv};
  const auto rows = traj_rows(c);
  for (size_t i = 0; i < rows.size(); i++)
    if (host[i]) HIPCHK(c, hipMemcpy(host[i], *rows[i].p, rows[i].bytes * cnt, hipMemcpyDeviceToHost));
  return WK_OK;
}

int wk_set_trajectory(wk_ctx* c, int horizon, const float* s, const float* a, const float* lp,
                      const float* r, const uint8_t* d, const float* v) {
  DevGuard dg_(c);
  if (!c || horizon <= 0 || horizon > c->T || !s || !a || !lp || !r || !d || !v) return WK_ERR_ARG;
  const size_t cnt = (size_t)c->n * horizon;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const void* const host[6] = {s, a, lp, r, d, v};
  const auto rows = traj_rows(c);
  for (size_t i = 0; i < 6; i++)
    HIPCHK(c, hipMemcpy(*rows[i].p, host[i], rows[i].bytes * cnt, hipMemcpyHostToDevice));
  c->T_valid = horizon;
  c->returns_valid = false;
  c->vlast_valid = false;
  // foreign data: scaled with the scale as it is, nothing learned (wk_reward_norm_update learns it)
  if (c->rn_on) return rnorm_pass(c, false);
  return WK_OK;
}

int wk_get_bootstrap_values(wk_ctx* c, float* v) {
  DevGuard dg_(c);
  if (!c || !v) return WK_ERR_ARG;
  if (c->cfg.ReturnsMode != 1) { SETERR(c, "wk_get_bootstrap_values needs ReturnsMode = 1"); return WK_ERR_STATE; }
  if (!c->vlast_valid) {
    SETERR(c, "no bootstrap values: call wk_rollout or wk_set_bootstrap_values first");
    return WK_ERR_STATE;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(v, c->vlast, sizeof(float) * c->n, hipMemcpyDeviceToHost));
  return WK_OK;
}

int wk_set_bootstrap_values(wk_ctx* c, const float* v) {
  DevGuard dg_(c);
  if (!c || !v) return WK_ERR_ARG;
  if (c->cfg.ReturnsMode != 1) { SETERR(c, "wk_set_bootstrap_values needs ReturnsMode = 1"); return WK_ERR_STATE; }
  if (c->T_valid <= 0) {
    SETERR(c, "wk_set_bootstrap_values before wk_rollout / wk_set_trajectory");
    return WK_ERR_STATE;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->vlast, v, sizeof(float) * c->n, hipMemcpyHostToDevice));
  c->vlast_valid = true;
  c->returns_valid = false;
  return WK_OK;
}

// ---------------- reward normalisation (wk_rnorm.hip) ----------------
static_assert(sizeof(wk_reward_norm) == sizeof(wk::RnormRec), "wk_reward_norm layout");

// var and scale from (count, m2, epsilon): the finish kernel's formula, on the host
static void rnorm_scale(wk::RnormRec& r, float epsilon) {
  r.var = r.count > 0 ? r.m2 / (double)r.count : 0.0;
  r.scale = 1.0f;
  if (r.count > 0) {
    const float sc = (float)(1.0 / std::sqrt(r.var + (double)epsilon));
    if (std::isfinite(sc) && sc > 0.0f) r.scale = sc;
  }
}

static int rnorm_need(wk_ctx* c, const char* fn) {
  if (c->rn_ever) return WK_OK;
  SETERR(c, "%s: reward normalisation was never enabled on this context (wk_reward_norm_config)", fn);
  return WK_ERR_STATE;
}

// the statistics changed under a trajectory: its returns are stale and its scaled rewards follow
static int rnorm_changed(wk_ctx* c) {
  if (c->T_valid <= 0) return WK_OK;
  c->returns_valid = false;
  return c->rn_on ? rnorm_pass(c, false) : WK_OK;
}

void wk_reward_norm_defaults(wk_reward_norm_args* a) {
  if (!a) return;
  a->enable = 0;
  a->frozen = 0;
  a->clip = 10.0f;
  a->epsilon = 1e-8f;
}

int wk_reward_norm_config(wk_ctx* c, const wk_reward_norm_args* a) {
  DevGuard dg_(c);
  if (!c || !a) return WK_ERR_ARG;
  if (a->enable < 0 || a->enable > 1 || a->frozen < 0 || a->frozen > 1 || !(a->clip > 0.0f) ||
      !std::isfinite(a->epsilon) || a->epsilon < 0.0f) {
    SETERR(c, "wk_reward_norm_config: enable and frozen are 0 or 1, clip > 0 (+inf: no clamp), epsilon "
              "finite and >= 0 (got %d, %d, %g, %g)", a->enable, a->frozen, (double)a->clip, (double)a->epsilon);
    return WK_ERR_ARG;
  }
  if (a->enable && (c->comm || c->host_ar || c->ipc || c->xch) && !records_on(c)) {
    SETERR(c, "reward normalisation is one GPU without wk_comm_records: this context has a gradient "
              "exchange, and every rank would scale by its own shard's statistics");
    return WK_ERR_CONFIG;
  }
  if (a->enable && !c->rn_ever) {  // the first enable: acc 0, no samples, scale 1
    const size_t n = c->n;
    if (!c->rn_acc) HIPCHK(c, dev_alloc(c, &c->rn_acc, sizeof(float) * n));
    if (!c->trs) HIPCHK(c, dev_alloc(c, &c->trs, sizeof(float) * n * c->T));
    if (!c->rn_rec) HIPCHK(c, dev_alloc(c, &c->rn_rec, sizeof(wk::RnormRec)));
    if (!c->rn_partial)
      HIPCHK(c, dev_alloc(c, &c->rn_partial, sizeof(unsigned long long) * wk::RNORM_FIELDS * wk::rnorm_tiles(c->n)));
    wk::RnormRec r{};
    r.scale = 1.0f;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(c->rn_acc, 0, sizeof(float) * n));
    HIPCHK(c, hipMemcpy(c->rn_rec, &r, sizeof r, hipMemcpyHostToDevice));
    c->rn_ever = true;
  }
  const bool changed = a->enable != c->rn_on || a->frozen != c->rn_frozen ||
                       memcmp(&a->clip, &c->rn_clip, sizeof(float)) != 0 ||
                       memcmp(&a->epsilon, &c->rn_eps, sizeof(float)) != 0;
  if (c->rn_ever && a->epsilon != c->rn_eps) {  // the scale follows its epsilon
    wk::RnormRec r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&r, c->rn_rec, sizeof r, hipMemcpyDeviceToHost));
    rnorm_scale(r, a->epsilon);
    HIPCHK(c, hipMemcpy(c->rn_rec, &r, sizeof r, hipMemcpyHostToDevice));
  }
  c->rn_on = a->enable;
  c->rn_frozen = a->frozen;
  c->rn_clip = a->clip;
  c->rn_eps = a->epsilon;
  return changed && c->rn_ever ? rnorm_changed(c) : WK_OK;
}

int wk_reward_norm_get(wk_ctx* c, wk_reward_norm* out) {
  DevGuard dg_(c);
  if (!c || !out) return WK_ERR_ARG;
  memset(out, 0, sizeof(*out));
  out->scale = 1.0f;
  if (!c->rn_ever) return WK_OK;
  if (int r = rx_deferred(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->rn_rec, sizeof(*out), hipMemcpyDeviceToHost));
  out->clip = c->rn_clip;
  out->epsilon = c->rn_eps;
  out->enabled = c->rn_on;
  out->frozen = c->rn_frozen;
  out->pad = 0;
  return WK_OK;
}

int wk_reward_norm_set(wk_ctx* c, int64_t count, double mean, double m2) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (int r = rnorm_need(c, "wk_reward_norm_set")) return r;
  if (count < 0 || !std::isfinite(mean) || !std::isfinite(m2) || m2 < 0.0) {
    SETERR(c, "wk_reward_norm_set: count >= 0, a finite mean and a finite m2 >= 0 (got %lld, %g, %g)",
           (long long)count, mean, m2);
    return WK_ERR_ARG;
  }
  wk::RnormRec r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&r, c->rn_rec, sizeof r, hipMemcpyDeviceToHost));
  r.count = count;
  r.mean = mean;
  r.m2 = m2;
  rnorm_scale(r, c->rn_eps);
  HIPCHK(c, hipMemcpy(c->rn_rec, &r, sizeof r, hipMemcpyHostToDevice));
  return rnorm_changed(c);
}

int wk_reward_norm_get_acc(wk_ctx* c, float* acc) {
  DevGuard dg_(c);
  if (!c || !acc) return WK_ERR_ARG;
  if (int r = rnorm_need(c, "wk_reward_norm_get_acc")) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(acc, c->rn_acc, sizeof(float) * c->n, hipMemcpyDeviceToHost));
  return WK_OK;
}

int wk_reward_norm_set_acc(wk_ctx* c, const float* acc) {
  DevGuard dg_(c);
  if (!c || !acc) return WK_ERR_ARG;
  if (int r = rnorm_need(c, "wk_reward_norm_set_acc")) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->rn_acc, acc, sizeof(float) * c->n, hipMemcpyHostToDevice));
  return WK_OK;
}

int wk_reward_norm_update(wk_ctx* c) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (int r = rnorm_need(c, "wk_reward_norm_update")) return r;
  if (c->T_valid <= 0) { SETERR(c, "wk_reward_norm_update: no trajectory recorded"); return WK_ERR_STATE; }
  c->returns_valid = false;
  return rnorm_pass(c, true);
}

int wk_get_scaled_rewards(wk_ctx* c, float* out) {
  DevGuard dg_(c);
  if (!c || !out) return WK_ERR_ARG;
  if (int r = rnorm_need(c, "wk_get_scaled_rewards")) return r;
  if (c->T_valid <= 0) { SETERR(c, "wk_get_scaled_rewards: no trajectory recorded"); return WK_ERR_STATE; }
  if (int r = rx_deferred(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->trs, sizeof(float) * c->n * c->T_valid, hipMemcpyDeviceToHost));
  return WK_OK;
}

// ---------------- data collection ----------------
static_assert(sizeof(wk_episode_rec) == sizeof(wk::EpisodeRecDev), "episode record layout");

int wk_collect_data(wk_ctx* c, int on) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  c->collect = on ? 1 : 0;
  return WK_OK;
}

int wk_episode_log_count(wk_ctx* c, int64_t* episodes, int64_t* updates) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  uint64_t cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, c->ep_count, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (episodes) *episodes = (int64_t)cnt;
  if (updates) *updates = (int64_t)c->loss_count;
  return WK_OK;
}

int wk_episode_log_drain(wk_ctx* c, wk_episode_rec* out, int64_t cap, int64_t* n_out,
                         int64_t* dropped) {
  DevGuard dg_(c);
  if (!c || cap < 0 || (cap > 0 && !out)) return WK_ERR_ARG;
  uint64_t cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, c->ep_count, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t kept = cnt < c->ep_cap ? cnt : c->ep_cap;
  if ((uint64_t)cap < kept) {
    SETERR(c, "episode log holds %llu records, buffer has room for %lld", (unsigned long long)kept, (long long)cap);
    return WK_ERR_ARG;
  }
  if (kept) HIPCHK(c, hipMemcpy(out, c->ep_log, sizeof(wk_episode_rec) * kept, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemsetAsync(c->ep_count, 0, sizeof(uint64_t), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->snap_log_drained = true;
  if (n_out) *n_out = (int64_t)kept;
  if (dropped) *dropped = (int64_t)(cnt - kept);
  return WK_OK;
}

int wk_loss_log_drain(wk_ctx* c, float* critic, float* actor, int64_t cap, int64_t* n_out,
                      int64_t* dropped) {
  DevGuard dg_(c);
  if (!c || cap < 0 || (cap > 0 && (!critic || !actor))) return WK_ERR_ARG;
  const uint64_t kept = c->loss_count < c->loss_cap ? c->loss_count : c->loss_cap;
  if ((uint64_t)cap < kept) {
    SETERR(c, "loss log holds %llu updates, buffer has room for %lld", (unsigned long long)kept, (long long)cap);
    return WK_ERR_ARG;
  }
  std::vector<float> buf(2 * kept);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (kept) HIPCHK(c, hipMemcpy(buf.data(), c->loss_log, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < kept; i++) {
    critic[i] = buf[2 * i];
    actor[i] = buf[2 * i + 1];
  }
  if (n_out) *n_out = (int64_t)kept;
  if (dropped) *dropped = (int64_t)(c->loss_count - kept);
  c->loss_count = 0;
  return WK_OK;
}

// ConsoleRenderer.CreateDataFile (ConsoleRenderer.cs:124-135): three space-joined float
// lists (float.ToString(), en-US) each followed by a "length N, <name>" line and a blank line
int wk_write_data_file(const char* path, const float* total_rewards, int64_t n_rewards,
                       const float* critic_losses, int64_t n_critic, const float* actor_losses,
                       int64_t n_actor) {
  if (!path || n_rewards < 0 || n_critic < 0 || n_actor < 0 ||
      (n_rewards && !total_rewards) || (n_critic && !critic_losses) || (n_actor && !actor_losses)) {
    wk::set_last_error("invalid argument");
    return WK_ERR_ARG;
  }
  std::string data;
  auto list = [&](const float* v, int64_t k, const char* name) {
    for (int64_t i = 0; i < k; i++) {
      if (i) data += ' ';
      data += wk::dotnet_float(v[i]);
    }
    data += "\nlength " + std::to_string(k) + ", " + name + "\n\n";
  };
  list(total_rewards, n_rewards, "total rewards");
  list(critic_losses, n_critic, "critic losses");
  list(actor_losses, n_actor, "actor losses");
  if (!write_file(path, data.data(), data.size())) {
    wk::set_last_error(std::string("cannot write '") + path + "'");
    return WK_ERR_ARG;
  }
  return WK_OK;
}
