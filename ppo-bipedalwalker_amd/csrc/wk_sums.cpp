// wk_sums.cpp -- the raw sums of the statistics passes as the ABI sees them (wk_ppo_sums): the
// fold step of the record exchange and the two divisions that turn sums into wk_ppo_stats and
// wk_log_std_grad.  Host arithmetic only: no context, no device, nothing but the public header, so
// tests/cpp/sums_check.cpp compiles this file for the host as it is.
#include <cstring>
#include <limits>

#include "../../include/wk_api.h"

static_assert(sizeof(wk_ppo_sums) == 8 * 13, "wk_ppo_sums is 13 64-bit words");

// acc = acc + x: integers add, doubles add, rmax is the larger with a NaN on either side staying
// (stats_add / stats_max of wk_stats.h, the device folds' step)
void wk_ppo_sums_add(wk_ppo_sums* acc, const wk_ppo_sums* x) {
  if (!acc || !x) return;
  acc->rows += x->rows;
  acc->skipped += x->skipped;
  acc->clipped += x->clipped;
  acc->kl += x->kl;
  acc->k1 += x->k1;
  acc->surr += x->surr;
  acc->sr += x->sr;
  acc->srr += x->srr;
  acc->se += x->se;
  acc->see += x->see;
  acc->rmax = (x->rmax > acc->rmax || x->rmax != x->rmax) ? x->rmax : acc->rmax;
  acc->term += x->term;
  acc->zz += x->zz;
}

// wk_ppo_stats from the sums: the host divides
void wk_ppo_stats_from_sums(const wk_ppo_sums* s, wk_ppo_stats* o) {
  if (!s || !o) return;
  const wk_ppo_sums& r = *s;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  memset(o, 0, sizeof(*o));
  o->samples = r.rows;
  o->skipped = r.skipped;
  const double n = (double)r.rows, ne = 4.0 * n;  // (0 / 0: every mean of no rows is NaN)
  o->kl = r.kl / ne;
  o->kl_k1 = r.k1 / ne;
  o->clip_fraction = (double)r.clipped / ne;
  o->ratio_max = r.rows > 0 ? r.rmax : nan;
  o->surrogate = r.surr / ne;
  o->value_loss = r.see / n;
  // population variances from the sums; a Var(ret) within the rounding of its own sums (n terms
  // of srr, each to 2^-53) is the variance of a constant: 0
  const double mr = r.sr / n, me = r.se / n;
  const double var_r = r.srr / n - mr * mr, var_e = r.see / n - me * me;
  const bool flat = var_r <= 4.0 * n * 0x1p-53 * (r.srr / n);
  o->explained_variance = (r.rows > 0 && !flat) ? 1.0 - var_e / var_r : nan;
  if (var_r != var_r) o->explained_variance = nan;
}

// wk_log_std_grad from the sums (0 / 0: no counted row gives NaN)
void wk_log_std_grad_from_sums(const wk_ppo_sums* s, float entropy_coef, wk_log_std_grad* ls) {
  if (!s || !ls) return;
  memset(ls, 0, sizeof(*ls));
  const double ne = 4.0 * (double)s->rows;
  ls->samples = s->rows;
  ls->skipped = s->skipped;
  ls->grad_surrogate = -s->term / ne;
  ls->grad = ls->grad_surrogate - (double)entropy_coef;
  ls->z2_mean = s->zz / ne;
}
