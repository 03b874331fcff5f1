// wk_eval.hip -- policy evaluation (wk_evaluate): per-walker episode accounting and the ordered
// fold of the episode records.
//
// The evaluation steps a private copy of the walkers with the kernels the rollout uses
// (wk_api_eval.cpp wk_evaluate: observations, policy kernel, one env-step of the physics kernel in its
// caller-actions mode).  After every env-step
//   k_eval_step    one lane per walker on SoA state (double reward sum, length, best x, episode
//                  index): adds the step; on `done` writes the slot's record with plain stores
//                  and restarts the sums; a walker past its last episode does nothing.  The count
//                  of walkers still running is kept with one integer atomic per wave (ballot +
//                  popcount, as k_episode_scan; an integer, so its value is order-independent).
// and once at the end
//   k_eval_fold    one lane per walker (its episode slots in episode order), striding over the
//                  walkers; a lane's record of EVAL_FIELDS 64-bit words goes to LDS, thread f folds
//                  field f over the lanes in lane order, then over the waves in wave order, and
//                  stores the block's word;
//   k_eval_finish  one block: thread f folds field f of the blocks' records in block order.
// Integers and doubles only, no floating-point atomics: the same records give the same bytes.
// The host divides (wk_api_eval.cpp).
// Traffic of k_eval_step per walker-step: 13 B of the physics row (reward, done, position x) and
// 32 B of running state read and written back -- about 45 B, next to a physics launch that moves the
// 448-B walker record both ways.
#include <hip/hip_runtime.h>

#include "wk_kernels.h"

namespace wk {

namespace {
constexpr int STEP_BLOCK = 256;
constexpr int FOLD_WAVES = EVAL_FOLD_BLOCK / 64;
constexpr float NEG_INF = -__builtin_inff();

__device__ __forceinline__ unsigned long long u64(long long v) { return (unsigned long long)v; }
__device__ __forceinline__ unsigned long long d64(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double as_d(unsigned long long v) { return __longlong_as_double((long long)v); }

// the larger / smaller of the two; a NaN on either side stays (wk_stats.h stats_max)
__device__ __forceinline__ double keep_max(double m, double v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double keep_min(double m, double v) { return (v < m || v != v) ? v : m; }

// field f of the fold's record: the empty value, and two words combined
__device__ __forceinline__ unsigned long long eval_zero(int f) {
  if (f == EF_RMIN) return d64((double)__builtin_inff());
  if (f == EF_RMAX || f == EF_DMAX) return d64(-(double)__builtin_inff());
  if (f == EF_LMIN) return u64(0x7fffffffll);
  if (f == EF_LMAX) return u64(-1ll);
  return 0ull;
}
__device__ __forceinline__ unsigned long long eval_add(unsigned long long a, unsigned long long b, int f) {
  if (f <= EF_LEN) return u64((long long)a + (long long)b);
  if (f <= EF_DIST) return d64(as_d(a) + as_d(b));
  if (f == EF_RMIN) return d64(keep_min(as_d(a), as_d(b)));
  if (f <= EF_DMAX) return d64(keep_max(as_d(a), as_d(b)));
  if (f == EF_LMIN) return u64((long long)a < (long long)b ? (long long)a : (long long)b);
  if (f == EF_LMAX) return u64((long long)a > (long long)b ? (long long)a : (long long)b);
  return a | b;
}
}  // namespace

// the start of an evaluation: empty running episodes, every slot UNFINISHED and zero otherwise,
// the private Philox counters at rng_step0, the fault row clear, every walker running
__global__ __launch_bounds__(STEP_BLOCK) void k_eval_init(EvalArgs a, uint32_t* __restrict__ rng_t,
                                                         uint32_t rng_step0, uint32_t* __restrict__ fault) {
  const int e = blockIdx.x * STEP_BLOCK + threadIdx.x;
  if (e == 0) *a.running = (uint32_t)a.n;
  if (e >= a.n) return;
  a.acc[e] = 0.0;
  a.len[e] = 0;
  a.best[e] = NEG_INF;
  a.epi[e] = 0;
  rng_t[e] = rng_step0;
  fault[e] = 0u;
  EvalRecDev z;
  z.total_reward = 0.0f; z.length = 0; z.distance = 0.0f; z.final_x = 0.0f;
  z.end = EVAL_UNFINISHED; z.env = 0;
  for (int k = 0; k < a.episodes; k++) a.recs[(size_t)k * a.n + e] = z;
}

__global__ __launch_bounds__(STEP_BLOCK) void k_eval_step(EvalArgs a) {
  const int e = blockIdx.x * STEP_BLOCK + threadIdx.x;
  const bool live = e < a.n;
  const int k = live ? a.epi[e] : a.episodes;
  const bool run = k < a.episodes;  // (false for a lane without a walker)
  bool last = false;
  if (run) {
    const double acc = a.acc[e] + (double)a.rew[e];
    const int len = a.len[e] + 1;
    const float x = a.pos[(size_t)e * 2];
    const float b0 = a.best[e];
    const float best = x > b0 ? x : b0;  // (a NaN x is ignored)
    if (a.done[e] != 0) {
      EvalRecDev r;
      r.total_reward = (float)acc;
      r.length = len;
      r.distance = best;
      r.final_x = x;
      r.end = x > 900.0f ? EVAL_SUCCESS : (len > a.max_timesteps ? EVAL_TIME_LIMIT : EVAL_FELL);
      r.env = a.env_offset + e;
      a.recs[(size_t)k * a.n + e] = r;
      a.acc[e] = 0.0;
      a.len[e] = 0;
      a.best[e] = NEG_INF;
      a.epi[e] = k + 1;
      last = k + 1 == a.episodes;
    } else {
      a.acc[e] = acc;
      a.len[e] = len;
      a.best[e] = best;
    }
  }
  const uint64_t b = __ballot(last);
  if (b && (threadIdx.x & 63) == 0) atomicSub(a.running, (uint32_t)__popcll(b));
}

__global__ __launch_bounds__(EVAL_FOLD_BLOCK) void k_eval_fold(const EvalRecDev* __restrict__ recs,
                                                              const uint32_t* __restrict__ fault, int n,
                                                              int episodes,
                                                              unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long rec[FOLD_WAVES * EVAL_FIELDS * 64];
  long long c_done = 0, c_unfin = 0, c_fell = 0, c_timed = 0, c_succ = 0, s_len = 0;
  double s_r = 0.0, s_rr = 0.0, s_d = 0.0;
  double rmin = (double)__builtin_inff(), rmax = -(double)__builtin_inff(), dmax = -(double)__builtin_inff();
  long long lmin = 0x7fffffffll, lmax = -1ll;
  unsigned long long f_or = 0ull;
  for (int e = blockIdx.x * EVAL_FOLD_BLOCK + threadIdx.x; e < n; e += gridDim.x * EVAL_FOLD_BLOCK) {
    f_or |= (unsigned long long)fault[e];
#pragma unroll 1
    for (int k = 0; k < episodes; k++) {
      const EvalRecDev r = recs[(size_t)k * n + e];
      if (r.end == EVAL_UNFINISHED) {
        c_unfin += 1;
        continue;
      }
      const double x = (double)r.total_reward, d = (double)r.distance;
      c_done += 1;
      c_fell += r.end == EVAL_FELL ? 1 : 0;
      c_timed += r.end == EVAL_TIME_LIMIT ? 1 : 0;
      c_succ += r.end == EVAL_SUCCESS ? 1 : 0;
      s_len += r.length;
      s_r += x;
      s_rr += x * x;
      s_d += d;
      rmin = keep_min(rmin, x);
      rmax = keep_max(rmax, x);
      dmax = keep_max(dmax, d);
      lmin = r.length < lmin ? r.length : lmin;
      lmax = r.length > lmax ? r.length : lmax;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* w = rec + (size_t)wave * EVAL_FIELDS * 64 + lane;
  w[EF_DONE * 64] = u64(c_done);
  w[EF_UNFIN * 64] = u64(c_unfin);
  w[EF_FELL * 64] = u64(c_fell);
  w[EF_TIMED * 64] = u64(c_timed);
  w[EF_SUCC * 64] = u64(c_succ);
  w[EF_LEN * 64] = u64(s_len);
  w[EF_R * 64] = d64(s_r);
  w[EF_RR * 64] = d64(s_rr);
  w[EF_DIST * 64] = d64(s_d);
  w[EF_RMIN * 64] = d64(rmin);
  w[EF_RMAX * 64] = d64(rmax);
  w[EF_DMAX * 64] = d64(dmax);
  w[EF_LMIN * 64] = u64(lmin);
  w[EF_LMAX * 64] = u64(lmax);
  w[EF_FAULT * 64] = f_or;
  __syncthreads();
  const int f = threadIdx.x;
  if (f >= EVAL_FIELDS) return;
  unsigned long long acc = eval_zero(f);
  for (int wv = 0; wv < FOLD_WAVES; wv++) {  // lanes in lane order, then the waves in wave order
    const unsigned long long* p = rec + ((size_t)wv * EVAL_FIELDS + f) * 64;
    unsigned long long wacc = eval_zero(f);
#pragma unroll 8
    for (int l = 0; l < 64; l++) wacc = eval_add(wacc, p[l], f);
    acc = eval_add(acc, wacc, f);
  }
  partial[(size_t)blockIdx.x * EVAL_FIELDS + f] = acc;
}

__global__ __launch_bounds__(64) void k_eval_finish(const unsigned long long* __restrict__ partial,
                                                   int nblocks, unsigned long long* __restrict__ out) {
  const int f = threadIdx.x;
  if (f >= EVAL_FIELDS) return;
  unsigned long long acc = eval_zero(f);
  for (int b = 0; b < nblocks; b++) acc = eval_add(acc, partial[(size_t)b * EVAL_FIELDS + f], f);
  out[f] = acc;
}

int eval_fold_blocks(int n) {
  const int b = (n + EVAL_FOLD_BLOCK - 1) / EVAL_FOLD_BLOCK;
  return b < 1 ? 1 : (b > EVAL_FOLD_MAX_BLOCKS ? EVAL_FOLD_MAX_BLOCKS : b);
}

hipError_t launch_eval_init(const EvalArgs& a, uint32_t* rng_t, uint32_t rng_step0, uint32_t* fault,
                            hipStream_t s) {
  k_eval_init<<<(a.n + STEP_BLOCK - 1) / STEP_BLOCK, STEP_BLOCK, 0, s>>>(a, rng_t, rng_step0, fault);
  return hipGetLastError();
}

hipError_t launch_eval_step(const EvalArgs& a, hipStream_t s) {
  k_eval_step<<<(a.n + STEP_BLOCK - 1) / STEP_BLOCK, STEP_BLOCK, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_eval_fold(const EvalRecDev* recs, const uint32_t* fault, int n, int episodes,
                            unsigned long long* partial, unsigned long long* out, hipStream_t s) {
  const int nb = eval_fold_blocks(n);
  k_eval_fold<<<nb, EVAL_FOLD_BLOCK, 0, s>>>(recs, fault, n, episodes, partial);
  k_eval_finish<<<1, 64, 0, s>>>(partial, nb, out);
  return hipGetLastError();
}

}  // namespace wk
