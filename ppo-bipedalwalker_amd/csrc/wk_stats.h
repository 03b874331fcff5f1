// wk_stats.h -- the arithmetic k_ppo_stats (wk_stats.hip) and k_net_stats (wk_net.hip) share:
// the per-entry statistics of one (row, action dimension), a lane's running sums, and the
// ordered folds lane -> wave -> block.  Device code only.
//
// LS (the log-std pass, wk_log_std_gradient and a LearnLogStd = 1 update) is a compile-time
// parameter of all of it: <false> is the statistics pass as it always was, <true> adds the
// derivative of the clipped surrogate by the log-std and two trailing double sums to the record.
#pragma once
#include <type_traits>

#include "wk_kernels.h"
#include "wk_mfma_layout.h"
#include "wk_ppo_math.h"

namespace wk {

template <bool LS>
constexpr int stats_fields() { return LS ? (int)STATS_FIELDS_LS : (int)STATS_FIELDS; }

// a lane's sums across its chunks, in chunk order: doubles, the counts as integers
struct StatsAccNone {};
struct StatsAccLS {
  double term = 0.0, zz = 0.0;  // w (zz - 1) and zz over the counted entries
};
template <bool LS>
struct StatsAcc : std::conditional<LS, StatsAccLS, StatsAccNone>::type {
  int rows = 0, skipped = 0, clipped = 0;
  double kl = 0.0, k1 = 0.0, surr = 0.0, sr = 0.0, srr = 0.0, se = 0.0, see = 0.0;
  float rmax = -__builtin_inff();
};

// the larger of the two; a NaN on either side stays
__device__ __forceinline__ double stats_max(double m, double v) { return (v > m || v != v) ? v : m; }

// One entry, in lane (row n, dim g) of a wave whose 64 lanes are all active: zz, lp, rr and the
// clipped surrogates are ppo_derivative's (wk_ppo_math.h, the function the gradient kernels call,
// PPOAgent.cs:234-326) in fp32, then d = lp - lpo in fp32 and everything after it in double.
// valid: the row exists; the skip rule (ppo_row_used: expf(lpo) == 0 in any of the row's four
// dimensions) decides with it whether the row counts.  Returns lp (for every row).
// LS: w = rr sel with ppo_derivative's sel = partA + partB partC, the gradient kernels' selection
// of the clipped surrogate's derivative by lp, in fp32; d lp / d log_std = zz - 1 with zz =
// ((act - mean) / std)^2; the entry's term (double)w ((double)zz - 1) and zz in double.
template <bool LS>
__device__ __forceinline__ float stats_entry(StatsAcc<LS>& a, const GradArgs& ga, bool valid, bool row_lane,
                                             float mean, float V, float act, float lpo, float ret,
                                             float adv) {
  // (the loss members are not read here, so `use` and eo, which only they depend on, are not the
  // skip rule's: that follows the terms, as it always did in this text)
  auto terms = [&] {
    return ppo_derivative(valid, mean, V, act, lpo, 1.0f, ret, adv, ga.std_, ga.lp_const, ga.upper, ga.lower, ga.b_div);
  };
  const PpoTerms t = terms();
  const float zz = t.zz, lp = t.lp, rr = t.rr, cra = t.cra, ra = t.ra;
  const float d = lp - lpo;
  const float sg = ra <= cra ? ra : cra;
  float eo;
  const bool use = ppo_row_used(valid, lpo, eo);
  if (use) {
    const double dd = (double)d;
    a.kl += expm1(dd) - dd;
    a.k1 += -dd;
    a.surr += (double)sg;
    a.clipped += (rr > ga.upper || rr < ga.lower) ? 1 : 0;
    a.rmax = (rr > a.rmax || rr != rr) ? rr : a.rmax;
    if constexpr (LS) {
      const float w = rr * terms().sel;  // (evaluated here, in the counted branch: the same value as t.sel)
      a.term += (double)w * ((double)zz - 1.0);
      a.zz += (double)zz;
    }
    if (row_lane) {
      const double r = (double)ret, e = r - (double)V;
      a.rows += 1;
      a.sr += r;
      a.srr += r * r;
      a.se += e;
      a.see += e * e;
    }
  } else if (valid && row_lane) {
    a.skipped += 1;
  }
  return lp;
}

// a lane's record into its wave's LDS image [stats_fields<LS>()][64] (64-bit words)
template <bool LS>
__device__ __forceinline__ void stats_put(const StatsAcc<LS>& a, unsigned long long* rec, int lane) {
  rec[0 * 64 + lane] = (unsigned long long)(long long)a.rows;
  rec[1 * 64 + lane] = (unsigned long long)(long long)a.skipped;
  rec[2 * 64 + lane] = (unsigned long long)(long long)a.clipped;
  const double v[7] = {a.kl, a.k1, a.surr, a.sr, a.srr, a.se, a.see};
#pragma unroll
  for (int i = 0; i < 7; i++) rec[(STATS_COUNTS + i) * 64 + lane] = (unsigned long long)__double_as_longlong(v[i]);
  rec[STATS_RMAX * 64 + lane] = (unsigned long long)__double_as_longlong((double)a.rmax);
  if constexpr (LS) {
    rec[(STATS_FIELDS + 0) * 64 + lane] = (unsigned long long)__double_as_longlong(a.term);
    rec[(STATS_FIELDS + 1) * 64 + lane] = (unsigned long long)__double_as_longlong(a.zz);
  }
}

// two words of field f combined: the counts as integers, the sums as doubles (the trailing
// words of the wide record among them), the maximum
__device__ __forceinline__ unsigned long long stats_zero(int f) {
  return f == STATS_RMAX ? (unsigned long long)__double_as_longlong(-(double)__builtin_inff()) : 0ull;
}
__device__ __forceinline__ unsigned long long stats_add(unsigned long long a, unsigned long long b, int f) {
  if (f < STATS_COUNTS) return (unsigned long long)((long long)a + (long long)b);
  const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
  return (unsigned long long)__double_as_longlong(f != STATS_RMAX ? x + y : stats_max(x, y));
}
// `n` records `stride` words apart, field f of each, folded in index order
__device__ __forceinline__ unsigned long long stats_fold(const unsigned long long* p, int n, int stride, int f) {
  unsigned long long acc = stats_zero(f);
#pragma unroll 8
  for (int i = 0; i < n; i++) acc = stats_add(acc, p[(size_t)i * stride], f);
  return acc;
}

// The block's record from its waves' LDS images rec[NW][NF][64], after a block barrier: thread
// f < NF folds field f of each wave's lanes in lane order, then the waves in wave order, and
// stores the block's word (a plain vector store).
template <int NW, int NF>
__device__ __forceinline__ void stats_block_fold(const unsigned long long* rec, int tid, unsigned long long* out) {
  if (tid >= NF) return;
  unsigned long long acc = stats_zero(tid);
#pragma unroll
  for (int w = 0; w < NW; w++) acc = stats_add(acc, stats_fold(rec + ((size_t)w * NF + tid) * 64, 64, 1, tid), tid);
  out[tid] = acc;
}

}  // namespace wk
