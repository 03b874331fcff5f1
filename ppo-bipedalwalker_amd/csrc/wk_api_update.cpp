// wk_api_update.cpp -- the PPO update: one minibatch's launch sequence, wk_ppo_update and the two
// single-batch calls, the statistics pass, the learned log-std's state and step, and the gradient
// kernel's timing.
#include <cmath>
#include <cstring>
#include <limits>

#include "wk_ctx.h"

// How many block slabs of what size g's gradient kernel (*gi) writes, and g.partial = c->partial
// sized for them.  Built-in kernels: nblocks slabs of SLAB floats (the sequential kernel: one);
// general kernels (always k_net_grad): nblocks slabs of slabn floats.
static int grad_slabs(wk_ctx* c, wk::GradArgs& g, bool sequential, int* gi, int* nblocks) {
  size_t floats;
  *gi = wk::grad_impl_for(c->grad_impl, g.samples);
  if (c->general) {
    *nblocks = wk::net_grad_blocks(g.samples);
    floats = (size_t)*nblocks * c->slabn;
  } else {
    *nblocks = sequential ? 1 : wk::ppo_grad_mfma_blocks(g.samples, *gi);
    floats = (size_t)*nblocks * wk::SLAB;
  }
  if (ensure(c, &c->partial, &c->partial_bytes, sizeof(float) * floats)) return WK_ERR_HIP;
  g.partial = c->partial;
  return WK_OK;
}

// the kernel family's matrix-core gradient kernel (the seam's other half, see launch_policy_for)
static hipError_t launch_grad_for(wk_ctx* c, const wk::GradArgs& g, int nblocks, int gi) {
  return c->general ? wk::launch_net_grad(g, c->net_dev, c->act_rows, c->np, c->stream)
                    : wk::launch_ppo_grad_mfma(g, nblocks, gi, c->stream);
}

static wk::AdamArgs adam_args(wk_ctx* c) {  // advances the step count
  wk::AdamArgs a{};
  c->adam_t += 1;
  const wk_config& k = c->cfg;
  a.W = c->W; a.m = c->m; a.v = c->v; a.grad = c->grad; a.Wz = c->Wz;
  a.c1 = 1.0f - k.Beta1;
  a.c2 = 1.0f - k.Beta2;
  a.beta1 = k.Beta1;
  a.beta2 = k.Beta2;
  a.bc1 = (float)(1.0 - pow((double)k.Beta1, (double)c->adam_t));
  a.bc2 = (float)(1.0 - pow((double)k.Beta2, (double)c->adam_t));
  a.alpha = k.Alpha;
  a.eps = k.AdamEpsilon;
  return a;
}

// MaxGradNorm > 0: the norms of the summed gradient in c->grad, the scaled Adam step and the
// device record in one launch (k_clip_adam), timed under the Adam slot
static int clip_adam(wk_ctx* c, const wk::AdamArgs& a) {
  ProfScope ps(c, PK_ADAM, 0, 2);
  HIPCHK(c, wk::launch_clip_adam(a, c->np, c->net.critic.n_params, c->cfg.MaxGradNorm, c->gnorm,
                                 c->stream));
  c->gnorm_steps += 1;
  return WK_OK;
}
// the record describes one wk_ppo_update / wk_train_batch / wk_minibatch_gradient: cleared,
// stream-ordered, at its start
static int gnorm_clear(wk_ctx* c) {
  if (!c->gnorm) return WK_OK;
  HIPCHK(c, hipMemsetAsync(c->gnorm, 0, sizeof(wk::GradNormRec), c->stream));
  c->gnorm_steps = 0;
  return WK_OK;
}

// one minibatch: gradient kernel -> ordered block reduction -> [RCCL all-reduce] -> Adam
// sequential: the lane-per-neuron kernel (wk_ppo.hip: one wave visits the samples in minibatch
// order) instead of the kernel family's matrix-core kernel; the general networks have no
// sequential kernel
static int minibatch(wk_ctx* c, wk::GradArgs g, bool sequential, int apply_adam) {
  int gi, nblocks;
  if (int r = grad_slabs(c, g, sequential, &gi, &nblocks)) return r;
  wk::AdamArgs a{};
  if (apply_adam) a = adam_args(c);
  // MaxGradNorm > 0: the reduction leaves Adam to k_clip_adam, which runs on the summed gradient
  const bool clip = apply_adam && c->gnorm != nullptr;
  {
    ProfScope ps(c, PK_GRAD, 0, 2);
    HIPCHK(c, sequential && !c->general ? wk::launch_ppo_grad(g, c->stream)
                                        : launch_grad_for(c, g, nblocks, gi));
  }
  // the general networks: the ordered sum of k_net_grad's block slabs with Adam in the same
  // launch (one GPU: the exchanges refuse such a context)
  if (c->general) {
    {
      ProfScope ps(c, PK_REDUCE, 0, 2);
      HIPCHK(c, wk::launch_net_reduce(c->partial, nblocks, c->np, c->grad, clip ? wk::AdamArgs{} : a,
                                      c->stream));
    }
    return clip ? clip_adam(c, a) : WK_OK;
  }
  // with a communicator (any size, also one rank) the collective path runs: reduction,
  // RCCL all-reduce, Adam -- a single-GPU test then covers the multi-GPU sequence
  const bool multi = c->comm != nullptr || c->host_ar != nullptr || c->ipc;
  // reduction, exchange and Adam in one launch (k_reduce_xch_adam); a gradient-only call
  // (apply_adam 0: a.W == null) runs the exchange alone, so on every kind of context the
  // returned gradient is the sum over the ranks
  if (c->ipc) {
    ProfScope ps(c, PK_ALLRED, 0, 2);
    wk::XchArgs x = c->xa;
    x.partial = c->partial;
    x.nblocks = nblocks;
    x.grad_out = c->grad;
    x.seq = ++c->xch_seq;
    x.err = c->xch_err;
    x.timeout_ticks = c->xch_timeout_ticks;
    x.t = (uint32_t)c->adam_t;
    x.a = a;
    x.stamps = xch_stamp_slot(c);
    HIPCHK(c, wk::launch_reduce_xch_adam(x, c->stream));
    return WK_OK;
  }
  const bool fused_adam = apply_adam && !multi && !clip;  // one GPU: the reduction applies Adam
  {
    ProfScope ps(c, PK_REDUCE, 0, 2);
    HIPCHK(c, wk::launch_grad_reduce(c->partial, nblocks, c->grad, fused_adam ? &a : nullptr,
                                     c->stream));
  }
  if (fused_adam) return WK_OK;

  if (multi)
    if (int r = comm_exchange(c)) return r;
  if (clip) return clip_adam(c, a);
  if (apply_adam) {
    ProfScope ps(c, PK_ADAM, 0, 2);
    HIPCHK(c, wk::launch_adam(a, c->stream));
  }
  return WK_OK;
}

static wk::GradArgs grad_base(wk_ctx* c) {
  wk::GradArgs g{};
  g.W = c->W;
  g.Wz = c->Wz;
  g.std_ = c->P.std_;
  g.lp_const = c->lp_const;
  g.upper = 1.0f + c->cfg.Epsilon;
  g.lower = 1.0f - c->cfg.Epsilon;
  return g;
}

// minibatches of M keyed samples out of the context's trajectory (the caller sets pk and base)
static wk::GradArgs traj_grad_args(wk_ctx* c, int M, float b_div) {
  wk::GradArgs g = grad_base(c);
  g.states = c->ts; g.actions = c->ta; g.logp_old = c->tlp; g.returns = c->tret; g.adv = c->tadv;
  g.pool = (uint32_t)((size_t)c->n * c->T_valid);
  g.use_perm = 1;
  g.samples = M;
  g.b_div = b_div;
  return g;
}

// the kernel family's statistics pass (the seam's third part, see launch_policy_for)
static int stats_blocks_for(wk_ctx* c, int rows) {
  return c->general ? wk::net_stats_blocks(rows) : wk::ppo_stats_blocks(rows);
}
static hipError_t launch_stats_for(wk_ctx* c, const wk::StatsArgs& a, int nblocks, bool log_std) {
  return c->general ? wk::launch_net_stats(a, c->net_dev, c->act_rows, log_std, c->stream)
                    : wk::launch_ppo_stats(a, nblocks, log_std, c->stream);
}

static_assert(sizeof(wk_ppo_sums) == sizeof(wk::StatsRecLS) && sizeof(wk_ppo_sums) == 8 * wk::STATS_FIELDS_LS &&
              8 * wk::STATS_FIELDS_LS < 8 * wk::RECORD_WORDS, "wk_ppo_sums is StatsRecLS, and fits a record");

// The statistics pass over the valid trajectory buffer with the current weights (wk_policy_stats
// and the per-epoch check of a TargetKL > 0 update): forward kernel, k_stats_finish, the record
// and the optional per-row outputs copied to the host.  Stale returns are computed first, and
// whether they count as valid is left as it was.
// wide: the log-std pass instead (wk_log_std_gradient, the LearnLogStd step) -- the kernels' wide
// instantiation, whose record holds the statistics' record too (the narrow pass leaves term and zz 0).
// global: on a record-exchange context (records_on) the pass is collective -- this rank's record
// goes through the gather behind a header, and *global is the ranks' records folded in rank order
// from rank 0's; the copy to the host the pass makes anyway is the gathered records'.
static int sums_impl(wk_ctx* c, bool wide, wk_ppo_sums* local, wk_ppo_sums* global, float* logp_new,
                     float* values_new) {
  if (c->T_valid <= 0) { SETERR(c, "wk_policy_stats before wk_rollout / wk_set_trajectory"); return WK_ERR_STATE; }
  if (global)
    if (int r = rx_deferred(c)) return r;
  if (!c->returns_valid) {
    int r = returns_impl(c);
    if (r) return r;
    c->returns_valid = false;
  }
  const size_t rows = (size_t)c->n * c->T_valid;
  if (rows > (size_t)INT32_MAX / 16) { SETERR(c, "wk_policy_stats: %zu rows exceed the kernel's index range", rows); return WK_ERR_ARG; }
  const int nblocks = stats_blocks_for(c, (int)rows);
  wk::StatsArgs a{};
  a.g = grad_base(c);
  a.g.states = c->ts; a.g.actions = c->ta; a.g.logp_old = c->tlp; a.g.returns = c->tret; a.g.adv = c->tadv;
  a.g.pool = (uint32_t)rows;
  a.g.samples = (int)rows;
  const size_t rec_bytes = wide ? sizeof(wk::StatsRecLS) : sizeof(wk::StatsRec);
  void* d_rec;
  if (carve(c, &c->scratch2, &c->scratch2_bytes,
            {{&a.partial, rec_bytes * (size_t)nblocks}, {&d_rec, rec_bytes},
             {&a.logp_new, logp_new ? sizeof(float) * 4 * rows : 0},
             {&a.values_new, values_new ? sizeof(float) * rows : 0}}))
    return WK_ERR_HIP;
  HIPCHK(c, launch_stats_for(c, a, nblocks, wide));
  HIPCHK(c, wk::launch_stats_finish(a.partial, nblocks, wide, d_rec, c->stream));
  memset(local, 0, sizeof(*local));
  if (global) {
    const uint64_t header = rx_header(c, 1);
    HIPCHK(c, wk::launch_record_pack(d_rec, (int)(rec_bytes / 8), header,
                                     c->rx_dev + (size_t)c->rank * wk::RECORD_WORDS, c->stream));
    if (int r = rx_gather_host(c, header)) return r;
    const auto rec_of = [&](int r) {
      wk_ppo_sums x;
      memcpy(&x, c->rx_host.data() + (size_t)r * wk::RECORD_WORDS + 1, sizeof x);
      return x;
    };
    *local = rec_of(c->rank);
    *global = rec_of(0);
    for (int r = 1; r < c->nranks; r++) {
      const wk_ppo_sums x = rec_of(r);
      wk_ppo_sums_add(global, &x);
    }
    return WK_OK;
  }
  HIPCHK(c, hipMemcpyAsync(local, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream));
  if (logp_new)
    HIPCHK(c, hipMemcpyAsync(logp_new, a.logp_new, sizeof(float) * 4 * rows, hipMemcpyDeviceToHost, c->stream));
  if (values_new)
    HIPCHK(c, hipMemcpyAsync(values_new, a.values_new, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

// this rank's shard: wk_policy_stats (ls null) and wk_log_std_gradient (the wide pass; out may be null)
static int stats_impl(wk_ctx* c, wk_ppo_stats* out, float* logp_new, float* values_new,
                      wk_log_std_grad* ls = nullptr) {
  wk_ppo_sums s;
  if (int r = sums_impl(c, ls != nullptr, &s, nullptr, logp_new, values_new)) return r;
  if (out) wk_ppo_stats_from_sums(&s, out);
  if (ls) wk_log_std_grad_from_sums(&s, c->cfg.EntropyCoef, ls);
  return WK_OK;
}

int wk_policy_sums(wk_ctx* c, wk_ppo_sums* local, wk_ppo_sums* global) {
  DevGuard dg_(c);
  if (!c || !local) return WK_ERR_ARG;
  const bool comm = c->comm || c->host_ar || c->ipc;
  if (global && comm && !records_on(c)) {
    SETERR(c, "wk_policy_sums: the global record needs the record exchange (wk_comm_records before the "
              "communicator)");
    return WK_ERR_STATE;
  }
  if (int r = sums_impl(c, true, local, comm ? global : nullptr, nullptr, nullptr)) return r;
  if (global && !comm) *global = *local;
  return WK_OK;
}

int wk_policy_stats_global(wk_ctx* c, wk_ppo_stats* out) {
  if (!c || !out) return WK_ERR_ARG;
  wk_ppo_sums local, global;
  if (int r = wk_policy_sums(c, &local, &global)) return r;
  wk_ppo_stats_from_sums(&global, out);
  return WK_OK;
}

int wk_log_std_gradient(wk_ctx* c, wk_log_std_grad* out) {
  DevGuard dg_(c);
  if (!c || !out) return WK_ERR_ARG;
  return stats_impl(c, nullptr, nullptr, nullptr, out);
}

int wk_get_log_std(wk_ctx* c, wk_log_std_state* out) {
  if (!c || !out) return WK_ERR_ARG;
  memset(out, 0, sizeof(*out));
  out->log_std = c->P.log_std;
  out->std = c->P.std_;
  out->entropy = (double)c->P.log_std + 0.5 * std::log(2.0 * 3.14159265358979323846 * 2.71828182845904523536);
  if (c->cfg.LearnLogStd != 1) return WK_OK;
  out->t = c->ls.t;
  out->m = c->ls.m;
  out->v = c->ls.v;
  out->grad_last = c->ls.grad_last;
  out->steps = c->ls.steps;
  out->clamped = c->ls.clamped;
  out->nonfinite = c->ls.nonfinite;
  return WK_OK;
}

int wk_set_log_std(wk_ctx* c, float log_std) {
  if (!c) return WK_ERR_ARG;
  if (!std::isfinite(log_std) || log_std <= -5.0f || log_std >= 5.0f) {
    SETERR(c, "wk_set_log_std: the log-std must be finite and inside (-5, 5)");
    return WK_ERR_ARG;
  }
  if (c->cfg.LearnLogStd == 1 && (log_std < c->cfg.LogStdMin || log_std > c->cfg.LogStdMax)) {
    SETERR(c, "wk_set_log_std: %g is outside [LogStdMin, LogStdMax] = [%g, %g]", (double)log_std,
           (double)c->cfg.LogStdMin, (double)c->cfg.LogStdMax);
    return WK_ERR_ARG;
  }
  apply_log_std(c, log_std);
  return WK_OK;
}

int wk_set_log_std_adam(wk_ctx* c, double m, double v, int t) {
  if (!c) return WK_ERR_ARG;
  if (c->cfg.LearnLogStd != 1) {
    SETERR(c, "wk_set_log_std_adam: the context does not train its log-std (LearnLogStd = 0)");
    return WK_ERR_STATE;
  }
  if (!std::isfinite(m) || !std::isfinite(v) || v < 0.0 || t < 0) {
    SETERR(c, "wk_set_log_std_adam: m and v must be finite, v and t not negative");
    return WK_ERR_ARG;
  }
  c->ls.m = m;
  c->ls.v = v;
  c->ls.t = t;
  return WK_OK;
}

// One Adam step on the scalar log-std, on the host in double, from the pass's record; a
// non-finite gradient (or no counted row: 0 / 0) takes no step and is counted
static void log_std_step(wk_ctx* c, const wk_log_std_grad& g) {
  c->ls.grad_last = g.grad;
  if (!std::isfinite(g.grad)) {
    c->ls.nonfinite++;
    return;
  }
  const double b1 = (double)c->cfg.Beta1, b2 = (double)c->cfg.Beta2, eps = (double)c->cfg.AdamEpsilon;
  const double lr = c->cfg.LogStdAlpha > 0.0f ? (double)c->cfg.LogStdAlpha : (double)c->cfg.Alpha;
  c->ls.m = b1 * c->ls.m + (1.0 - b1) * g.grad;
  c->ls.v = b2 * c->ls.v + (1.0 - b2) * g.grad * g.grad;
  c->ls.t += 1;
  const double mh = c->ls.m / (1.0 - std::pow(b1, (double)c->ls.t));
  const double vh = c->ls.v / (1.0 - std::pow(b2, (double)c->ls.t));
  const float s = (float)((double)c->P.log_std - lr * mh / (std::sqrt(vh) + eps));
  const float sc = std::min(std::max(s, c->cfg.LogStdMin), c->cfg.LogStdMax);
  if (sc != s) c->ls.clamped++;
  c->ls.steps++;
  apply_log_std(c, sc);
}

int wk_policy_stats(wk_ctx* c, wk_ppo_stats* out, float* logp_new, float* values_new) {
  DevGuard dg_(c);
  if (!c || !out) return WK_ERR_ARG;
  return stats_impl(c, out, logp_new, values_new);
}

int wk_update_stats_get(wk_ctx* c, wk_ppo_stats* out) {
  if (!c || !out) return WK_ERR_ARG;
  if (!c->upd_stats_valid) {
    SETERR(c, "wk_update_stats_get: the last wk_ppo_update made no check (TargetKL = 0, or no update yet)");
    return WK_ERR_STATE;
  }
  *out = c->upd_stats;
  return WK_OK;
}

int wk_grad_norms_get(wk_ctx* c, wk_grad_norms* out) {
  DevGuard dg_(c);
  if (!c || !out) return WK_ERR_ARG;
  static_assert(sizeof(wk_grad_norms) == sizeof(wk::GradNormRec), "the device record is wk_grad_norms");
  if (!c->gnorm || c->gnorm_steps == 0) {
    SETERR(c, "wk_grad_norms_get: no Adam step was measured (MaxGradNorm = 0, or no step since the "
              "record was cleared)");
    return WK_ERR_STATE;
  }
  HIPCHK(c, hipMemcpyAsync(out, c->gnorm, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_grad_kernel(wk_ctx* c, int minibatch) {
  if (!c || minibatch < 0) return WK_ERR_ARG;
  if (c->general) return 4;  // k_net_grad
  return wk::grad_impl_for(c->grad_impl, minibatch > 0 ? minibatch : c->cfg.Minibatch);
}

// The gradient kernel alone, `reps` back-to-back launches on minibatch 0 of the keyed sequence
// (update 0, epoch 0) of the current trajectory, between one HIP-event pair on the context's
// stream: the kernel's mean duration without per-launch event overhead (bench.py's update
// roofline; the launches write only the scratch slabs, no weights change)
int wk_time_gradient(wk_ctx* c, int minibatch, int reps, double* ms_per_launch) {
  return wk_time_gradient_ex(c, minibatch, reps, 0, ms_per_launch);
}

int wk_time_gradient_ex(wk_ctx* c, int minibatch, int reps, int flags, double* ms_per_launch) {
  DevGuard dg_(c);
  if (!c || reps <= 0 || !ms_per_launch || (flags & ~1)) return WK_ERR_ARG;
  if (c->T_valid <= 0) { SETERR(c, "wk_time_gradient before wk_rollout / wk_set_trajectory"); return WK_ERR_STATE; }
  if (!c->returns_valid) {
    int r = returns_impl(c);
    if (r) return r;
  }
  const int M = minibatch > 0 ? minibatch : c->cfg.Minibatch;
  const uint32_t pool = (uint32_t)((size_t)c->n * c->T_valid);
  if ((uint32_t)M > pool) { SETERR(c, "minibatch %d larger than the pool %u", M, pool); return WK_ERR_ARG; }
  wk::GradArgs g = traj_grad_args(c, M, (float)(c->cfg.MinibatchGlobal > 0 ? c->cfg.MinibatchGlobal : M));
  g.pk = wk::perm_key(c->seed, 0u, 0u, pool);
  int gi, nblocks;
  if (int r = grad_slabs(c, g, false, &gi, &nblocks)) return r;
  HIPCHK(c, launch_grad_for(c, g, nblocks, gi));  // warm
  // flags & 1: an event pair around EVERY launch (as profile level 2 times the update's
  // launches), the elapsed times summed -- the burst's per-launch event overhead is the
  // difference to one pair around the whole burst
  const int npairs = (flags & 1) ? reps : 1;
  // the events stay in the context's pool (nothing below draws from it): no path has to free them
  while (c->pool.size() < 2 * (size_t)npairs) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->pool.push_back(e);
  }
  const hipEvent_t* ev = c->pool.data() + c->pool.size() - 2 * (size_t)npairs;
  for (int i = 0; i < reps; i++) {
    if ((flags & 1) || i == 0) HIPCHK(c, hipEventRecord(ev[2 * ((flags & 1) ? i : 0)], c->stream));
    HIPCHK(c, launch_grad_for(c, g, nblocks, gi));
    if ((flags & 1) || i == reps - 1) HIPCHK(c, hipEventRecord(ev[2 * ((flags & 1) ? i : 0) + 1], c->stream));
  }
  HIPCHK(c, hipEventSynchronize(ev[2 * npairs - 1]));
  double total = 0.0;
  for (int i = 0; i < npairs; i++) {
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    total += ms;
  }
  *ms_per_launch = total / reps;
  return WK_OK;
}

static int ppo_update_impl(wk_ctx* c, const wk_ppo_args* args) {
  c->upd_stats_valid = false;
  c->ls.steps = c->ls.clamped = c->ls.nonfinite = 0;
  if (!c->returns_valid) {
    int r = returns_impl(c);
    if (r) return r;
  }
  if (int r = xch_mark_t(c)) return r;
  if (int r = gnorm_clear(c)) return r;
  const int epochs = (args && args->epochs > 0) ? args->epochs : c->cfg.Epochs;
  const int M = (args && args->minibatch > 0) ? args->minibatch : c->cfg.Minibatch;
  int Mg = (args && args->minibatch_global > 0) ? args->minibatch_global : c->cfg.MinibatchGlobal;
  if (Mg <= 0) Mg = M * c->nranks;
  const uint32_t update = args ? args->update_index : 0u;
  const uint32_t pool = (uint32_t)((size_t)c->n * c->T_valid);
  const int nmb = (int)(pool / (uint32_t)M);  // remainder dropped (PPOAgent.cs:506)
  if (nmb <= 0) { SETERR(c, "minibatch %d larger than the pool %u", M, pool); return WK_ERR_ARG; }
  wk::GradArgs g = traj_grad_args(c, M, (float)Mg);
  for (int e = 0; e < epochs; e++) {
    g.pk = wk::perm_key(c->seed, update, (uint32_t)e, pool);
    for (int j = 0; j < nmb; j++) {
      g.base = (uint32_t)j * (uint32_t)M;
      int r = minibatch(c, g, false, 1);
      if (r) return r;
    }
    // TargetKL: the policy's distance from the one that collected the data, after every epoch
    // (the last included); past the target the remaining epochs are not run (a NaN never stops)
    // LearnLogStd: the same pass, widened, yields the log-std's gradient as well (one pass per
    // epoch, not two); the step on the scalar comes before the stop decision, and g takes the new
    // std for the next epoch's gradient kernels
    // On a record-exchange context the pass's record is gathered and folded over the ranks: the
    // step and the decision are taken from the same bytes on every rank (one exchange per epoch).
    const bool learn = c->cfg.LearnLogStd == 1;
    const bool check = c->cfg.TargetKL > 0.0f;
    if (records_on(c) && (learn || check)) {
      wk_ppo_sums local, global;
      if (int r = sums_impl(c, learn, &local, &global, nullptr, nullptr)) return r;
      if (check) wk_ppo_stats_from_sums(&global, &c->upd_stats);
      if (learn) {
        wk_log_std_grad lg;
        wk_log_std_grad_from_sums(&global, c->cfg.EntropyCoef, &lg);
        log_std_step(c, lg);
        g.std_ = c->P.std_;
        g.lp_const = c->lp_const;
      }
    } else if (learn) {
      wk_log_std_grad lg;
      if (int r = stats_impl(c, check ? &c->upd_stats : nullptr, nullptr, nullptr, &lg)) return r;
      log_std_step(c, lg);
      g.std_ = c->P.std_;
      g.lp_const = c->lp_const;
    }
    if (check) {
      if (!learn && !records_on(c))
        if (int r = stats_impl(c, &c->upd_stats, nullptr, nullptr)) return r;
      const bool stop = c->upd_stats.kl > (double)c->cfg.TargetKL;
      c->upd_stats.epochs_run = e + 1;
      c->upd_stats.stopped_early = (stop && e + 1 < epochs) ? 1 : 0;
      c->upd_stats_valid = true;
      if (stop) break;
    }
  }
  return WK_OK;
}

int wk_ppo_update(wk_ctx* c, const wk_ppo_args* args, float* critic_diag, float* actor_diag) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (c->T_valid <= 0) { SETERR(c, "wk_ppo_update before wk_rollout / wk_set_trajectory"); return WK_ERR_STATE; }
  {
    ProfScope ps(c, PK_UPDATE);
    int r = ppo_update_impl(c, args);
    if (r) return r;
  }
  {  // a peer that never published is fatal for the job (like a failed all-reduce)
    int r = xch_status(c);
    if (r) return r;
  }
  if (c->collect) {  // the last minibatch's losses, as PPOAgent.Train hands them on (:165-166)
    if (c->loss_count < c->loss_cap)
      HIPCHK(c, hipMemcpyAsync(c->loss_log + 2 * c->loss_count, c->grad + c->np,
                               2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    c->loss_count++;
  }
  if (!critic_diag && !actor_diag) return WK_OK;  // stays asynchronous on the stream
  float diag[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(diag, c->grad + c->np, sizeof(diag), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (critic_diag) *critic_diag = diag[0];
  if (actor_diag) *actor_diag = diag[1];
  return WK_OK;
}

// sequential: as minibatch (wk_train_batch: the reference's sequential sums)
static int batch_impl(wk_ctx* c, bool sequential, int B, float b_div, const float* s, const float* a,
                      const float* lpo, const float* ret, const float* adv, float* cd, float* ad,
                      float* grads_out, int apply_adam, int* skipped) {
  if (!c || B <= 0 || !s || !a || !lpo || !ret || !adv) return WK_ERR_ARG;
  const size_t bs = sizeof(float) * B;
  float *d_s, *d_a, *d_l, *d_r, *d_v;
  if (carve(c, &c->scratch2, &c->scratch2_bytes,
            {{&d_s, bs * 12}, {&d_a, bs * 4}, {&d_l, bs * 4}, {&d_r, bs}, {&d_v, bs}}))
    return WK_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(d_s, s, bs * 12, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_a, a, bs * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_l, lpo, bs * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_r, ret, bs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_v, adv, bs, hipMemcpyHostToDevice, c->stream));
  wk::GradArgs g = grad_base(c);
  g.states = d_s; g.actions = d_a; g.logp_old = d_l; g.returns = d_r; g.adv = d_v;
  g.pool = (uint32_t)B;
  g.base = 0;
  g.use_perm = 0;
  g.samples = B;
  g.b_div = b_div;
  int r = xch_mark_t(c);
  if (r) return r;
  r = gnorm_clear(c);
  if (r) return r;
  r = minibatch(c, g, sequential, apply_adam);
  if (r) return r;
  std::vector<float> slab(c->slabn);
  HIPCHK(c, hipMemcpyAsync(slab.data(), c->grad, sizeof(float) * slab.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  r = xch_status(c);  // (IPC: a timed-out exchange left grad stale and applied no Adam)
  if (r) return r;
  if (grads_out) memcpy(grads_out, slab.data(), sizeof(float) * c->np);
  if (cd) *cd = slab[c->np];
  if (ad) *ad = slab[c->np + 1];
  if (skipped) *skipped = (int)slab[c->np + 2];
  return WK_OK;
}

int wk_train_batch(wk_ctx* c, int B, float b_div, const float* s, const float* a, const float* lpo,
                   const float* ret, const float* adv, float* cd, float* ad, float* grads_out,
                   int apply_adam, int* skipped) {
  DevGuard dg_(c);
  return batch_impl(c, true, B, b_div, s, a, lpo, ret, adv, cd, ad, grads_out, apply_adam, skipped);
}

int wk_minibatch_gradient(wk_ctx* c, int B, float b_div, const float* s, const float* a,
                          const float* lpo, const float* ret, const float* adv, float* cd,
                          float* ad, float* grads_out, int* skipped) {
  DevGuard dg_(c);
  return batch_impl(c, false, B, b_div, s, a, lpo, ret, adv, cd, ad, grads_out, 0, skipped);
}
