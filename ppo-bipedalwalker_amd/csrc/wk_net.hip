// wk_net.hip -- the general networks' kernels (NetworkKernels = 1): any valid critic / actor
// string within wk_net.h's limits, layer widths as runtime values (gfx950).
//
// Mapping: one wave per block works on tiles of 16 samples.  A tile's activations live in LDS as
// one [row = neuron][16 samples] image per layer boundary (row stride 17 floats), every boundary
// kept: the forward pass is the cache NeuralNetwork.FeedForward keeps for FeedBack
// (NeuralNetwork.cs:52-82).  Dense layers run on v_mfma_f32_16x16x4_f32 (exact fp32 products and
// sums, a k-ordered fma chain; cdna_hip_programming lane maps: A[l & 15][l >> 4], B[l >> 4][l & 15],
// D[4 (l >> 4) + r][l & 15]):
//   forward   Z[out][s]  = W[out][in] X[in][s]        A = W (HBM / L2), B = X (LDS)
//   backward  Gx[in][s]  = W^T[in][out] G[out][s]     A = W^T,          B = G (LDS)
//   weights   dW[out][in] += G[out][s] X^T[s][in]     A = G,  B = X^T (LDS), C = the running sum
// Ragged widths are padded with zero operands (out to 16, in to 4); a zero product adds exactly
// nothing.  Accumulators and operand fragments are indexed by constants only: no scratch.
//
// Gradient sums: block b owns the tiles [b tpb, (b + 1) tpb) and visits them in order; dW / db
// accumulate in the block's own slab in HBM (at most NET_MAX_BLOCKS blocks) -- each lane reads and
// writes back the same elements every tile, the tile's 16 samples entering as the next k steps
// of the fma chain -- and the
// slabs are summed in block order by k_net_reduce (groups of RG, then the groups).  No atomics:
// the same inputs give the same bits.  Samples outside the minibatch (the ragged last tile) and
// samples the skip rule drops (Matrix.HadamardDivision throws on exp(logp_old) == 0 ->
// `continue`, PPOAgent.cs) enter with a zero state and a zero output gradient.
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_net.h"
#include "wk_sample.h"
#include "wk_stats.h"

namespace wk {

#define DEV __device__ __forceinline__

namespace nt {
enum : int {
  NS = 16,            // samples per tile
  LS = 17,            // floats per LDS row
  GROWS = NET_MAX_WIDTH,
  // per-tile sample fields [.][16]
  M_A = 0, M_LPO = 64, M_RET = 128, M_ADV = 144, M_OK = 160, M_SKIP = 176, M_ZERO = 192,
  M_CL = 256, M_AL = 272, M_END = 336
};
}  // namespace nt

typedef float nf4 __attribute__((ext_vector_type(4)));
DEV nf4 net_mfma(float a, float b, nf4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
enum : int { NACC = 8 };  // independent accumulator chains of one dot product
DEV nf4 net_tree(const nf4 (&p)[NACC]) {
  return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}

// ActivationLayer.cs:39-72
DEV float net_act(int kind, float z) {
  if (kind == NL_RELU) return z > 0.0f ? z : (z != z ? z : 0.0f);  // MathF.Max(0, z)
  if (kind == NL_LRELU) return z < 0.0f ? 0.2f * z : z;            // MathF.Max(0.2 z, z)
  return tanhf(z);
}
DEV float net_dact(int kind, float z) {
  if (kind == NL_RELU) return z < 0.0f ? 0.0f : 1.0f;
  if (kind == NL_LRELU) return z < 0.0f ? 0.2f : 1.0f;
  const float th = tanhf(z);
  return 1.0f - (th * th);
}

// NeuralNetwork.FeedForward with cache: rows [0, 12) of `act` hold the tile's states; every
// layer writes its output image.  The one forward routine of k_net_policy and k_net_grad.
DEV void net_forward(const NetDesc* __restrict__ d, const float* __restrict__ W, float* act, int lane) {
  using namespace nt;
  const int n = lane & 15, g = lane >> 4;
  const int nl = d->n_layers;
#pragma unroll 1
  for (int l = 0; l < nl; l++) {
    const NetLayer L = d->layer[l];
    const float* X = act + L.row_in * LS;
    float* Y = act + L.row_out * LS;
    if (L.kind == NL_DENSE) {
      // DenseLayer.FeedForward (DenseLayer.cs:82-98): z = (W x) + b
      const int ksteps = (L.in + 3) >> 2, mtiles = (L.out + 15) >> 4;
#pragma unroll 1
      for (int mt = 0; mt < mtiles; mt++) {
        const int o = 16 * mt + n;
        const bool orow = o < L.out;
        const float* wrow = W + L.off_w + (size_t)(orow ? o : 0) * L.in;
        // NACC independent fma chains (k steps j, j + NACC, ...) folded as a tree: the dot
        // product's rounding error grows with the chain length, and the chains hide the
        // MFMA's dependent latency; a step past the width multiplies zeros
        nf4 pa[NACC];
#pragma unroll
        for (int j = 0; j < NACC; j++) pa[j] = nf4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int kq = 0; kq < ksteps; kq += NACC) {
          float a[NACC], b[NACC];
#pragma unroll
          for (int j = 0; j < NACC; j++) {
            const int i = 4 * (kq + j) + g;
            const bool in = i < L.in;
            a[j] = (orow && in) ? wrow[i] : 0.0f;
            b[j] = in ? X[i * LS + n] : 0.0f;
          }
#pragma unroll
          for (int j = 0; j < NACC; j++) pa[j] = net_mfma(a[j], b[j], pa[j]);
        }
        const nf4 acc = net_tree(pa);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int oo = 16 * mt + 4 * g + r;
          if (oo < L.out) Y[oo * LS + n] = acc[r] + W[L.off_b + oo];
        }
      }
    } else {
      for (int idx = lane; idx < L.in * NS; idx += 64) {
        const int at = (idx >> 4) * LS + (idx & 15);
        Y[at] = net_act(L.kind, X[at]);
      }
    }
    __syncthreads();
  }
}

// NeuralNetwork.FeedBack (NeuralNetwork.cs:67-82) for one tile: `gin` holds dL/d(output)
// [n_out][16]; DenseLayer.FeedBack (DenseLayer.cs:103-120) adds dW = G X^T and db into the
// block's slab and hands W^T G on, ActivationLayer.FeedBack (:18-21) multiplies by the
// derivative at the cached input.  first: the block's first tile starts the sums at zero.
DEV void net_backward(const NetDesc* __restrict__ d, const float* __restrict__ W, const float* act,
                      float* gin, float* gout, float* slab, bool first, int lane) {
  using namespace nt;
  const int n = lane & 15, g = lane >> 4;
#pragma unroll 1
  for (int l = d->n_layers - 1; l >= 0; l--) {
    const NetLayer L = d->layer[l];
    const float* X = act + L.row_in * LS;
    if (L.kind != NL_DENSE) {
      for (int idx = lane; idx < L.in * NS; idx += 64) {
        const int at = (idx >> 4) * LS + (idx & 15);
        gin[at] = gin[at] * net_dact(L.kind, X[at]);
      }
      __syncthreads();
      continue;
    }
    const int otiles = (L.out + 15) >> 4, itiles = (L.in + 15) >> 4;
#pragma unroll 1
    for (int ot = 0; ot < otiles; ot++) {
      const int oa = 16 * ot + n;  // this lane's row of the A operand (G)
      const bool oa_ok = oa < L.out;
#pragma unroll 1
      for (int it = 0; it < itiles; it++) {
        const int ib = 16 * it + n;  // this lane's column of the B operand (X^T), and of D
        const bool ib_ok = ib < L.in;
        nf4 acc;
        int at[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int oo = 16 * ot + 4 * g + r;
          at[r] = (oo < L.out && ib_ok) ? L.off_w + oo * L.in + ib : -1;
          acc[r] = (first || at[r] < 0) ? 0.0f : slab[at[r]];
        }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const int s = 4 * kk + g;
          const float a = oa_ok ? gin[oa * LS + s] : 0.0f;
          const float b = ib_ok ? X[ib * LS + s] : 0.0f;
          acc = net_mfma(a, b, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (at[r] >= 0) slab[at[r]] = acc[r];
      }
    }
    for (int o = lane; o < L.out; o += 64) {
      float s = first ? 0.0f : slab[L.off_b + o];
#pragma unroll
      for (int c = 0; c < NS; c++) s = s + gin[o * LS + c];
      slab[L.off_b + o] = s;
    }
    if (l == 0) break;  // nothing reads the gradient of the states
    const int ksteps = (L.out + 3) >> 2;
#pragma unroll 1
    for (int it = 0; it < itiles; it++) {
      const int i = 16 * it + n;
      const bool icol = i < L.in;
      nf4 pa[NACC];
#pragma unroll
      for (int j = 0; j < NACC; j++) pa[j] = nf4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
      for (int kq = 0; kq < ksteps; kq += NACC) {
        float a[NACC], b[NACC];
#pragma unroll
        for (int j = 0; j < NACC; j++) {
          const int o = 4 * (kq + j) + g;
          const bool ok = o < L.out;
          a[j] = (ok && icol) ? W[L.off_w + (size_t)o * L.in + i] : 0.0f;
          b[j] = ok ? gin[o * LS + n] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NACC; j++) pa[j] = net_mfma(a[j], b[j], pa[j]);
      }
      const nf4 acc = net_tree(pa);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int ii = 16 * it + 4 * g + r;
        if (ii < L.in) gout[ii * LS + n] = acc[r];
      }
    }
    __syncthreads();
    float* t = gin; gin = gout; gout = t;
  }
  __syncthreads();
}

// n observations -> actor mean, sampled action and per-dimension log-density, critic value
// (PPOAgent.SampleActions PPOAgent.cs:381-398, GetValueEstimate :350-364); any output may be
// null.  nets[0] the critic, nets[1] the actor.
__global__ __launch_bounds__(64) void k_net_policy(EnvParams P, const NetDesc* __restrict__ nets,
                                                   const float* __restrict__ W, float lp_const, int n,
                                                   const float* __restrict__ obs,
                                                   const int32_t* __restrict__ env_ids,
                                                   const uint32_t* __restrict__ steps, float* mean_out,
                                                   float* act_out, float* logp_out, float* v_out) {
  using namespace nt;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* act = lds;
  const int lane = threadIdx.x, s = lane & 15, g = lane >> 4;
  const int i = blockIdx.x * NS + s;
  const bool live = i < n;
#pragma unroll
  for (int j = 0; j < 3; j++) act[(3 * g + j) * LS + s] = live ? obs[(size_t)i * 12 + 3 * g + j] : 0.0f;
  __syncthreads();
  if (mean_out || act_out || logp_out) {
    const NetDesc* a = nets + 1;
    net_forward(a, W, act, lane);
    if (g == 0 && live) {
      const float* out = act + a->row_end * LS;
      float mean[4], ac[4], lp[4];
#pragma unroll
      for (int dd = 0; dd < 4; dd++) mean[dd] = out[dd * LS + s];
      const uint32_t gid = env_ids ? (uint32_t)env_ids[i] : (uint32_t)(P.env_offset + i);
      const uint32_t t = steps ? steps[i] : 0u;
      sample_actions(P, lp_const, gid, t, mean, ac, lp);
#pragma unroll
      for (int dd = 0; dd < 4; dd++) {
        if (mean_out) mean_out[(size_t)i * 4 + dd] = mean[dd];
        if (act_out) act_out[(size_t)i * 4 + dd] = ac[dd];
        if (logp_out) logp_out[(size_t)i * 4 + dd] = lp[dd];
      }
    }
    __syncthreads();
  }
  if (v_out) {
    net_forward(nets, W, act, lane);
    if (g == 0 && live) v_out[i] = act[nets->row_end * LS + s];
  }
}

// Policy statistics over the trajectory (wk_policy_stats) for the general networks: k_net_policy's
// tile set-up, net_forward on the actor and then on the critic over the same LDS image, and the
// per-entry arithmetic and double records of wk_stats.h (lane (s, d): dimension d of row s).
// Block b owns the consecutive tiles [b tpb, (b + 1) tpb), as in k_net_grad, and writes one
// record; k_stats_finish (wk_stats.hip) sums the records in block order.  Every row is evaluated,
// the skipped ones too (their log-densities and values are outputs); a row's column of the
// activation image never meets another row's.  LSTD: the log-std pass (wk_stats.h's LS; here
// LS is the image's stride), same tiles; its two instantiations are the kernels k_net_stats
// (<false>, as it always was) and k_net_logstd (<true>) below.
template <bool LSTD>
__device__ __forceinline__ void net_stats_pass(const StatsArgs& sa, const NetDesc* __restrict__ nets,
                                               int act_rows, int tiles_per_block) {
  using namespace nt;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GradArgs& ga = sa.g;
  float* act = lds;
  const int lane = threadIdx.x, s = lane & 15, d = lane >> 4;
  const NetDesc* critic = nets;
  const NetDesc* actor = nets + 1;
  const int ntiles = (ga.samples + NS - 1) / NS;
  const int t0 = blockIdx.x * tiles_per_block;
  const int t1 = min(t0 + tiles_per_block, ntiles);
  StatsAcc<LSTD> acc;
#pragma unroll 1
  for (int tile = t0; tile < t1; tile++) {
    const int pos = tile * NS + s;
    const bool live = pos < ga.samples;
    const size_t idx = live ? (size_t)pos : 0;
    const float lpo = ga.logp_old[idx * 4 + d], ac = ga.actions[idx * 4 + d];
    const float ret = ga.returns[idx], adv = ga.adv[idx];
#pragma unroll
    for (int j = 0; j < 3; j++) act[(3 * d + j) * LS + s] = live ? ga.states[idx * 12 + 3 * d + j] : 0.0f;
    __syncthreads();
    net_forward(actor, ga.W, act, lane);
    const float mean = act[(actor->row_end + d) * LS + s];
    __syncthreads();  // the means are read before the critic's layers overwrite the image
    net_forward(critic, ga.W, act, lane);
    const float V = act[critic->row_end * LS + s];
    const float lp = stats_entry(acc, ga, live, d == 0, mean, V, ac, lpo, ret, adv);
    if (live) {
      if (sa.logp_new) sa.logp_new[(size_t)pos * 4 + d] = lp;
      if (sa.values_new && d == 0) sa.values_new[pos] = V;
    }
    __syncthreads();  // the next tile rewrites the image
  }
  unsigned long long* rec = (unsigned long long*)(lds + ((act_rows * LS + 1) & ~1));
  constexpr int NF = stats_fields<LSTD>();
  stats_put(acc, rec, lane);
  __syncthreads();
  stats_block_fold<1, NF>(rec, lane, sa.partial + (size_t)blockIdx.x * NF);
}

__global__ __launch_bounds__(64) void k_net_stats(StatsArgs sa, const NetDesc* __restrict__ nets,
                                                  int act_rows, int tiles_per_block) {
  net_stats_pass<false>(sa, nets, act_rows, tiles_per_block);
}
__global__ __launch_bounds__(64) void k_net_logstd(StatsArgs sa, const NetDesc* __restrict__ nets,
                                                   int act_rows, int tiles_per_block) {
  net_stats_pass<true>(sa, nets, act_rows, tiles_per_block);
}

struct NetGradArgs {
  GradArgs g;
  const NetDesc* nets;   // [0] critic, [1] actor
  int np, slabn;         // parameters; floats per slab (np + 3 diagnostics, padded to 4)
  int tiles_per_block;
  int act_rows;          // rows of the activation cache: max over the two networks
};

// PPOAgent.Train(Batch) (PPOAgent.cs:218-346) for the general network
__global__ __launch_bounds__(64) void k_net_grad(NetGradArgs A) {
  using namespace nt;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GradArgs& ga = A.g;
  float* act = lds;
  float* g0 = act + A.act_rows * LS;
  float* g1 = g0 + GROWS * LS;
  float* smp = g1 + GROWS * LS;
  const int lane = threadIdx.x, s = lane & 15, d = lane >> 4;
  float* slab = ga.partial + (size_t)blockIdx.x * A.slabn;
  const NetDesc* critic = A.nets;
  const NetDesc* actor = A.nets + 1;
  const int ntiles = (ga.samples + NS - 1) / NS;
  const int t0 = blockIdx.x * A.tiles_per_block;
  const int t1 = min(t0 + A.tiles_per_block, ntiles);
  float diagC = 0.0f, diagA = 0.0f, skipped = 0.0f;  // (lane 0)

#pragma unroll 1
  for (int tile = t0; tile < t1; tile++) {
    const bool first = tile == t0;
    // ---- gather the tile (CreateBatches, PPOAgent.cs:512-533) ----
    const int pos = tile * NS + s;
    const bool live = pos < ga.samples;
    uint32_t idx = 0;
    if (live) {
      idx = ga.base + (uint32_t)pos;
      if (ga.use_perm) idx = perm_apply(idx, ga.pk);
    }
    const float lpo = live ? ga.logp_old[(size_t)idx * 4 + d] : 0.0f;
    smp[M_LPO + lane] = lpo;
    smp[M_A + lane] = live ? ga.actions[(size_t)idx * 4 + d] : 0.0f;
    smp[M_ZERO + lane] = expf(lpo) == 0.0f ? 1.0f : 0.0f;
    if (d == 0) smp[M_RET + s] = live ? ga.returns[idx] : 0.0f;
    if (d == 1) smp[M_ADV + s] = live ? ga.adv[idx] : 0.0f;
    __syncthreads();
    const bool skip = live && (smp[M_ZERO + s] + smp[M_ZERO + 16 + s] + smp[M_ZERO + 32 + s] +
                               smp[M_ZERO + 48 + s]) != 0.0f;
    const bool ok = live && !skip;
    if (d == 0) { smp[M_OK + s] = ok ? 1.0f : 0.0f; smp[M_SKIP + s] = skip ? 1.0f : 0.0f; }
#pragma unroll
    for (int j = 0; j < 3; j++) act[(3 * d + j) * LS + s] = ok ? ga.states[(size_t)idx * 12 + 3 * d + j] : 0.0f;
    __syncthreads();

    // ---- critic: value, loss derivative, backward ----
    net_forward(critic, ga.W, act, lane);
    if (d == 0) {
      const float V = act[critic->row_end * LS + s];
      float criticLoss = 2.0f * (V - smp[M_RET + s]);
      criticLoss /= ga.b_div;
      criticLoss = ok ? criticLoss : 0.0f;
      g0[s] = criticLoss;
      smp[M_CL + s] = criticLoss;
    }
    __syncthreads();
    net_backward(critic, ga.W, act, g0, g1, slab, first, lane);

    // ---- actor: mean, the per-dimension clipped-surrogate derivative (:248-326), backward.
    // (ppo_derivative's text, wk_ppo_math.h, kept here: the critic's half is taken in other lanes
    // above and the skip is selected after the division; called through the function this kernel
    // compiles to other code -- DESIGN.md "One derivative") ----
    net_forward(actor, ga.W, act, lane);
    {
      const float mean = act[(actor->row_end + d) * LS + s];
      const float Adv = smp[M_ADV + s];
      const float ac = smp[M_A + lane];
      float fr = (ac - mean) / ga.std_;
      fr *= fr;
      fr /= 2.0f;
      const float lp = ga.lp_const - fr;
      const float r = expf(lp - lpo);
      const float cr = r >= ga.upper ? ga.upper : (r <= ga.lower ? ga.lower : r);
      const float cra = cr * Adv, ra = r * Adv;
      const float partA = (ra <= cra ? 1.0f : 0.0f) * Adv;
      const float partB = (cra < ra ? 1.0f : 0.0f) * Adv;
      const float partC = (r >= ga.lower && r <= ga.upper) ? 1.0f : 0.0f;
      float lo = partA + (partB * partC);
      lo = lo * -1.0f;
      const float lcd = lo / expf(lpo);
      const float prob = expf(lp);
      const float frac = (ac - mean) / (ga.std_ * ga.std_);
      float actorLoss = (prob * frac) * lcd;
      actorLoss = actorLoss / ga.b_div;
      actorLoss = ok ? actorLoss : 0.0f;
      g0[d * LS + s] = actorLoss;
      smp[M_AL + lane] = actorLoss;
    }
    __syncthreads();
    if (lane == 0) {  // the diagnostics, in sample order
#pragma unroll 1
      for (int c = 0; c < NS; c++) {
        if (smp[M_OK + c] != 0.0f) {
          diagC += smp[M_CL + c];
          diagA += ((((0.0f + smp[M_AL + c]) + smp[M_AL + 16 + c]) + smp[M_AL + 32 + c]) + smp[M_AL + 48 + c]) / 4.0f;
        }
        skipped += smp[M_SKIP + c];
      }
    }
    net_backward(actor, ga.W, act, g0, g1, slab, first, lane);
  }
  if (lane == 0) {
    slab[A.np] = diagC;
    slab[A.np + 1] = diagA;
    slab[A.np + 2] = skipped;
    for (int p = A.np + 3; p < A.slabn; p++) slab[p] = 0.0f;
  }
}

// Xavier-normal init (Matrix.FromXavier, Matrix.cs:59-80) on the device, for both kernel families
// (a built-in context passes the default strings' descriptions): element k of the l-th dense
// layer (critic first) draws philox(seed, k, l, 0, ST_XAVIER); biases are zero.  The two
// descriptions travel by value as kernel arguments, so the launch reads no device copy of them.
__global__ void k_xavier(float* W, uint64_t seed, NetDesc critic, NetDesc actor, int np) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  float v = 0.0f;
  int gl = 0;
  for (int q = 0; q < 2; q++) {
    const NetDesc* d = q == 0 ? &critic : &actor;
    for (int l = 0; l < d->n_layers; l++) {
      const NetLayer L = d->layer[l];
      if (L.kind != NL_DENSE) continue;
      if (p >= L.off_w && p < L.off_w + L.out * L.in) {
        const int k = p - L.off_w;
        U4 o = philox(seed, (uint32_t)k, (uint32_t)gl, 0, ST_XAVIER);
        float u1 = next_double_f(o.x, o.y), u2 = next_double_f(o.z, o.w);
        if (u1 == 0.0f) u1 = 1.0f;
        const float PI_F = 3.14159265358979323846f;
        float std_ = sqrtf(2.0f / (float)(L.out + L.in));
        float z = sqrtf(-2.0f * logf(u1)) * sinf(2.0f * PI_F * u2);
        v = 0.0f + (std_ * z);
      }
      gl++;
    }
  }
  W[p] = v;
}

// ---- host side ----
static size_t policy_lds(int act_rows) { return sizeof(float) * (size_t)act_rows * nt::LS; }
static size_t stats_lds(int act_rows) {
  // (the wide record's room for both instantiations: one size, one attribute)
  return sizeof(float) * (size_t)((act_rows * nt::LS + 1) & ~1) + sizeof(unsigned long long) * STATS_FIELDS_LS * 64;
}
static size_t grad_lds(int act_rows) {
  return sizeof(float) * ((size_t)(act_rows + 2 * nt::GROWS) * nt::LS + nt::M_END);
}

hipError_t configure_net_kernels() {
  const int rows = NET_STATE + NET_MAX_LAYERS * NET_MAX_WIDTH;  // the largest cache
  hipError_t e = hipFuncSetAttribute((const void*)k_net_grad, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)grad_lds(rows));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)k_net_policy, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_lds(rows));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)k_net_stats, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)stats_lds(rows));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)k_net_logstd, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)stats_lds(rows));
  return e;
}

int net_act_rows(const NetDesc& critic, const NetDesc& actor) {
  return critic.rows > actor.rows ? critic.rows : actor.rows;
}

hipError_t launch_net_policy(const EnvParams& P, const NetDesc* nets, int act_rows, const float* W,
                             float lp_const, int n, const float* obs, const int32_t* env_ids,
                             const uint32_t* steps, float* mean, float* act, float* logp, float* v,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_net_policy, dim3((n + nt::NS - 1) / nt::NS), dim3(64), policy_lds(act_rows), s, P,
                     nets, W, lp_const, n, obs, env_ids, steps, mean, act, logp, v);
  return hipGetLastError();
}

int net_slab_floats(int np) { return (np + 3 + 3) / 4 * 4; }

// the fixed assignment of sample tiles to blocks: at most NET_MAX_BLOCKS blocks of equally many
// consecutive tiles (every block has at least one)
static int net_tiles_per_block(int samples) {
  const int ntiles = (samples + nt::NS - 1) / nt::NS;
  return (ntiles + NET_MAX_BLOCKS - 1) / NET_MAX_BLOCKS;
}
int net_grad_blocks(int samples) {
  const int ntiles = (samples + nt::NS - 1) / nt::NS;
  const int tpb = net_tiles_per_block(samples);
  return (ntiles + tpb - 1) / tpb;
}

hipError_t launch_net_grad(const GradArgs& g, const NetDesc* nets, int act_rows, int np, hipStream_t s) {
  NetGradArgs A{};
  A.g = g;
  A.nets = nets;
  A.np = np;
  A.slabn = net_slab_floats(np);
  A.tiles_per_block = net_tiles_per_block(g.samples);
  A.act_rows = act_rows;
  hipLaunchKernelGGL(k_net_grad, dim3(net_grad_blocks(g.samples)), dim3(64), grad_lds(act_rows), s, A);
  return hipGetLastError();
}

// the statistics pass: k_net_grad's assignment of tiles to blocks
int net_stats_blocks(int rows) { return net_grad_blocks(rows); }

hipError_t launch_net_stats(const StatsArgs& a, const NetDesc* nets, int act_rows, bool log_std,
                            hipStream_t s) {
  const dim3 grid(net_stats_blocks(a.g.samples));
  const int tpb = net_tiles_per_block(a.g.samples);
  hipLaunchKernelGGL(log_std ? k_net_logstd : k_net_stats, grid, dim3(64), stats_lds(act_rows), s, a, nets,
                     act_rows, tpb);
  return hipGetLastError();
}

hipError_t launch_xavier(float* W, uint64_t seed, const NetDesc& critic, const NetDesc& actor, int np,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_xavier, dim3((np + 255) / 256), dim3(256), 0, s, W, seed, critic, actor, np);
  return hipGetLastError();
}

}  // namespace wk
