// wk_api_eval.cpp -- wk_evaluate and its timing (kernels: wk_eval.hip)
#include <cmath>
#include <cstring>
#include <limits>

#include "wk_ctx.h"

// ---------------- policy evaluation (wk_evaluate) ----------------
// The host divides the fold's sums; with no finished episode every mean and extremum is NaN.
static void eval_from_rec(const unsigned long long* w, wk_eval_stats* o) {
  const auto i64 = [&](int f) { return (int64_t)w[f]; };
  const auto f64 = [&](int f) { double d; memcpy(&d, &w[f], sizeof d); return d; };
  const double nan = std::numeric_limits<double>::quiet_NaN();
  o->episodes = i64(wk::EF_DONE);
  o->unfinished = i64(wk::EF_UNFIN);
  o->fell = i64(wk::EF_FELL);
  o->timed_out = i64(wk::EF_TIMED);
  o->succeeded = i64(wk::EF_SUCC);
  const bool any = o->episodes > 0;
  const double cnt = (double)o->episodes;  // (0 / 0: every mean of no episodes is NaN)
  const double mr = f64(wk::EF_R) / cnt;
  o->reward_mean = mr;
  o->reward_std = std::sqrt(std::max(0.0, f64(wk::EF_RR) / cnt - mr * mr));
  if (!any) o->reward_std = nan;  // (max(0, NaN) is 0)
  o->reward_min = any ? f64(wk::EF_RMIN) : nan;
  o->reward_max = any ? f64(wk::EF_RMAX) : nan;
  o->length_mean = (double)i64(wk::EF_LEN) / cnt;
  o->length_min = any ? (int32_t)i64(wk::EF_LMIN) : 0;
  o->length_max = any ? (int32_t)i64(wk::EF_LMAX) : 0;
  o->distance_mean = f64(wk::EF_DIST) / cnt;
  o->distance_max = any ? f64(wk::EF_DMAX) : nan;
  o->fault_or = (uint32_t)w[wk::EF_FAULT];
}

// Every walker of the context plays complete episodes under the current actor on a private copy of
// the walker state; per env-step the launches of net_sampled (observations, policy kernel, one
// env-step of the context's physics kernel in caller-actions mode) on that copy, then the
// accounting kernel.  No ProfScope and no context buffer but the private block and the pacing
// tags: nothing a later call can observe changes.
int wk_evaluate(wk_ctx* c, const wk_eval_args* args, wk_eval_stats* out, wk_eval_rec* recs) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  wk_eval_args g{};
  if (args) g = *args;
  if (!out) { SETERR(c, "wk_evaluate: out is NULL"); return WK_ERR_ARG; }
  if (g.episodes < 0 || g.episodes > WK_EVAL_MAX_EPISODES) {
    SETERR(c, "wk_evaluate: episodes %d outside 1..%d", g.episodes, (int)WK_EVAL_MAX_EPISODES);
    return WK_ERR_ARG;
  }
  if (g.max_steps < 0 || g.poll < 0) { SETERR(c, "wk_evaluate: negative max_steps or poll"); return WK_ERR_ARG; }
  if (g.start < 0 || g.start > 1 || g.stochastic < 0 || g.stochastic > 1) {
    SETERR(c, "wk_evaluate: start and stochastic are 0 or 1");
    return WK_ERR_ARG;
  }
  const int K = g.episodes ? g.episodes : 1;
  const int poll = g.poll ? g.poll : 32;
  const int64_t full = (int64_t)K * ((int64_t)c->cfg.MaxTimesteps + 1);
  const int max_steps = g.max_steps ? g.max_steps : (int)std::min<int64_t>(full, INT32_MAX);
  const size_t n = c->n, f = sizeof(float) * n;
  const bool props = c->scene.n_props > 0;
  // a private lane order only where launch_physics builds one (the flat floor's episode-0
  // partition); the rough floor's is static by start offset, which is the context's
  const bool own_order = c->order && !c->P.rough && !props;
  const int nblocks = wk::eval_fold_blocks(c->n);
  wk_ctx::EvalBlock& b = c->evb;
  b.valid = false;
  wk::EvalArgs& a = b.a;
  if (carve(c, &c->ev, &c->ev_bytes,
            {{&b.st, wk::NSTATE * f}, {&b.rng_t, sizeof(uint32_t) * n},
             {&b.props, props ? f * c->scene.pstride : 0},
             {&b.order, own_order ? sizeof(int32_t) * 3 * n : 0},
             {&b.order_cnt, own_order ? sizeof(uint32_t) * wk::order_cells(c->n) : 0},
             {&b.obs, 12 * f}, {&b.act, 4 * f}, {&b.rew, f}, {&b.pos, 2 * f}, {&b.done, n},
             {&b.fault, sizeof(uint32_t) * n},
             {&a.acc, sizeof(double) * n}, {&a.len, sizeof(int32_t) * n}, {&a.best, f},
             {&a.epi, sizeof(int32_t) * n}, {&a.recs, sizeof(wk::EvalRecDev) * n * K},
             {&a.running, sizeof(uint32_t)},
             {&b.partial, sizeof(unsigned long long) * wk::EVAL_FIELDS * nblocks},
             {&b.out, sizeof(unsigned long long) * wk::EVAL_FIELDS}}))
    return WK_ERR_HIP;
  a.n = c->n; a.episodes = K; a.env_offset = c->cfg.EnvOffset; a.max_timesteps = c->cfg.MaxTimesteps;
  a.rew = b.rew; a.done = b.done; a.pos = b.pos;
  // the walkers: the template in episode-0 order (the episode counter 0), then, for start 0, what
  // wk_reset(NULL) makes of it
  HIPCHK(c, wk::launch_env_init(c->P, b.st, c->dxoff, nullptr, 0, c->stream));
  if (g.start == 0) HIPCHK(c, wk::launch_env_init(c->P, b.st, c->dxoff, nullptr, 1, c->stream));
  if (props)
    HIPCHK(c, hipMemcpyAsync(b.props, c->props, f * c->scene.pstride, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, wk::launch_eval_init(a, b.rng_t, g.rng_step0, b.fault, c->stream));
  int steps = 0;
  uint32_t running = (uint32_t)c->n;
  while (steps < max_steps && running) {
    const int chunk = std::min(poll, max_steps - steps);
    for (int j = 0; j < chunk; j++) {
      HIPCHK(c, wk::launch_get_obs(c->P, b.st, b.obs, c->stream));
      HIPCHK(c, launch_policy_for(c, c->n, b.obs, nullptr, b.rng_t, g.stochastic ? nullptr : b.act,
                                  g.stochastic ? b.act : nullptr, nullptr, nullptr));
      wk::StepArgs A{};
      A.st = b.st; A.dxoff = c->dxoff; A.mat = c->mat; A.rng_t = b.rng_t;
      A.actions = b.act;
      A.rew_out = b.rew; A.done_out = b.done; A.pos_out = b.pos; A.fault_out = b.fault;
      A.k_steps = 1;
      HIPCHK(c, launch_physics(c, 0, A, b.props, own_order ? b.order : c->order, own_order ? b.order_cnt : c->order_cnt));
      HIPCHK(c, wk::launch_eval_step(a, c->stream));
    }
    steps += chunk;
    HIPCHK(c, hipMemcpyAsync(&running, a.running, sizeof(running), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, wk::launch_eval_fold(a.recs, b.fault, c->n, K, b.partial, b.out, c->stream));
  unsigned long long w[wk::EVAL_FIELDS];
  HIPCHK(c, hipMemcpyAsync(w, b.out, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  if (recs)
    HIPCHK(c, hipMemcpyAsync(recs, a.recs, sizeof(wk_eval_rec) * n * K, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  b.valid = true;
  memset(out, 0, sizeof(*out));
  eval_from_rec(w, out);
  out->steps_run = steps;
  out->env_steps = (int64_t)steps * c->n;
  return WK_OK;
}
static_assert(sizeof(wk_eval_rec) == sizeof(wk::EvalRecDev), "wk_eval_rec layout");

int wk_evaluate_time(wk_ctx* c, int reps, double* step_ms, double* fold_ms) {
  DevGuard dg_(c);
  if (!c || reps <= 0 || !step_ms || !fold_ms) return WK_ERR_ARG;
  wk_ctx::EvalBlock& b = c->evb;
  if (!b.valid) { SETERR(c, "wk_evaluate_time before wk_evaluate"); return WK_ERR_STATE; }
  while (c->pool.size() < 2) {  // the events stay in the context's pool, as in wk_time_gradient_ex
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->pool.push_back(e);
  }
  const hipEvent_t e0 = c->pool[c->pool.size() - 2], e1 = c->pool[c->pool.size() - 1];
  const auto burst = [&](bool fold, double* ms_out) -> int {
    for (int i = -1; i < reps; i++) {  // (i = -1: warm)
      if (i == 0) HIPCHK(c, hipEventRecord(e0, c->stream));
      HIPCHK(c, fold ? wk::launch_eval_fold(b.a.recs, b.fault, c->n, b.a.episodes, b.partial, b.out, c->stream)
                     : wk::launch_eval_step(b.a, c->stream));
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / reps;
    return WK_OK;
  };
  if (int r = burst(true, fold_ms)) return r;
  // the walkers run again: the accounting kernel does nothing for one past its last episode.  A
  // burst longer than the episodes asked for would finish them on the row's done flags, so the
  // row's flags are cleared too
  b.valid = false;
  HIPCHK(c, wk::launch_eval_init(b.a, b.rng_t, 0u, b.fault, c->stream));
  HIPCHK(c, hipMemsetAsync(b.done, 0, (size_t)c->n, c->stream));
  return burst(false, step_ms);
}
