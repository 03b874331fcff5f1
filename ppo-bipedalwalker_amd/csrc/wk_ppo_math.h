// wk_ppo_math.h -- the PPO clipped-surrogate derivative (PPOAgent.Train(Batch),
// PPOAgent.cs:234-326) and its skip rule, written once for the kernels on the built-in
// networks' weight image: the matrix-core gradient kernels (wk_ppo_mfma.hip) and, through
// stats_entry (wk_stats.h), the statistics and log-std passes of both network families.
// The sequential kernel (wk_ppo.hip) and the general networks' (wk_net.hip) keep their own
// text of it, for the reason given there.  Device code only.
//
// Everything here is a function of scalars in fp32 with the reference's operation order:
// nothing is re-associated or fused.  The configuration values (std, the log-density's
// constant, the clip bounds, the batch divisor) are taken by value: a caller passes its
// kernel argument's fields.
#pragma once
#include "wk_mfma_layout.h"

namespace wk {

// The skip rule, in lane (row n, dim g) of a wave whose 64 lanes are all active:
// Matrix.HadamardDivision throws on exp(logp_old) == 0, so the reference skips a row with
// such an entry in any of its four dimensions before it touches it.  valid: the row exists.
// Returns whether the row is used; eo = expf(lpo) of this lane's entry.
__device__ __forceinline__ bool ppo_row_used(bool valid, float lpo, float& eo) {
  eo = expf(lpo);
  float zd = eo == 0.0f ? 1.0f : 0.0f;
  zd = rows_max4(zd);
  return valid && zd == 0.0f;
}

// One (row, action dimension):
//   zz = ((act - mean) / std)^2, the log-density lp = lp_const - zz / 2, the ratio rr =
//   exp(lp - lpo), the surrogates ra = rr adv and cra = clip(rr) adv;
//   sel = partA + partB partC, the reference's selection of d min(ra, cra) / d rr;
//   critic = 2 (V - ret) and actor = (prob frac) (-sel / eo), the loss derivatives by V and by
//   the mean before the batch divisor and the skip rule (eo = expf(lpo), the divisor
//   Matrix.HadamardDivision refuses at 0);
//   criticLoss, actorLoss: those divided by the batch divisor, selected to zero for a row that
//   is not used; gz3 = actorLoss (1 - tanh(z3)^2) with mean = tanh(z3) (the reference takes the
//   tanh again in its backward pass: the same value).
// One straight function on purpose: a caller reads the members it needs and does not pay for
// the others, and the matrix-core kernels' machine code is the one their own copies of this
// text gave (split into nested helpers it was not: profiles/one_derivative_isa.txt).
struct PpoTerms { float zz, lp, rr, cra, ra, sel, critic, actor, criticLoss, actorLoss, gz3; };
__device__ __forceinline__ PpoTerms ppo_derivative(bool use, float mean, float V, float act, float lpo, float eo,
                                                   float ret, float adv, float std_, float lp_const,
                                                   float upper, float lower, float b_div) {
  float criticLoss = 2.0f * (V - ret);
  const float critic = criticLoss;
  float fr = (act - mean) / std_;
  fr *= fr;
  const float zz = fr;
  fr /= 2.0f;
  const float lp = lp_const - fr;
  const float rr = expf(lp - lpo);
  const float cr = rr >= upper ? upper : (rr <= lower ? lower : rr);
  const float cra = cr * adv, ra = rr * adv;
  const float partA = (ra <= cra ? 1.0f : 0.0f) * adv;
  const float partB = (cra < ra ? 1.0f : 0.0f) * adv;
  const float partC = (rr >= lower && rr <= upper) ? 1.0f : 0.0f;
  const float sel = partA + (partB * partC);
  float l = sel;
  l = l * -1.0f;
  const float lcd = l / eo;
  const float prob = expf(lp);
  const float frac = (act - mean) / (std_ * std_);
  float actorLoss = (prob * frac) * lcd;
  const float actor = actorLoss;
  criticLoss = use ? criticLoss / b_div : 0.0f;
  actorLoss = use ? actorLoss / b_div : 0.0f;
  const float th = mean;
  const float gz3 = actorLoss * (1.0f - (th * th));
  return {zz, lp, rr, cra, ra, sel, critic, actor, criticLoss, actorLoss, gz3};
}

}  // namespace wk
