// wk_stats.hip -- policy statistics over the trajectory for the built-in networks (gfx950):
// k_ppo_stats, a forward-only pass of the current actor and critic over every row of the buffer
// with the per-entry statistics of wk_stats.h behind it, and k_stats_finish, the ordered sum of
// the blocks' records (both kernel families); and k_ppo_logstd, the same pass instantiated with
// the log-std's derivative (wk_log_std_gradient, the LearnLogStd step).
//
// The forward pass is k_ppo_grad_mfma's forward half restated (wk_ppo_mfma.hip: the weight image
// Wz staged into LDS once per block, one wave per chunk of 16 rows, layer 1 and 2 on
// v_mfma_f32_16x16x4_f32 with layer 1's D registers as layer 2's B operand, the output rows as
// 64-long dots on the VALU, lane (n, g) ending with z3 of dimension g and V of row n), so a row's
// mean, log-density and value are the gradient kernel's bit for bit.  The only LDS tile a forward
// pass needs is SX.  Rows are read in buffer order; the grid is capped (STATS_MAX_BLOCKS) and the
// waves stride over the chunks, the next chunk's rows in flight during the math.
//
// Sums: each lane keeps its sums in double across its chunks in chunk order (counts as integers),
// a wave's lanes fold in lane order, a block's waves in wave order, and k_stats_finish sums the
// blocks' records in block order.  No atomics: the same inputs give the same bytes.
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_mfma_layout.h"
#include "wk_stats.h"

namespace wk {

#define DEV __device__ __forceinline__
typedef float f4 __attribute__((ext_vector_type(4)));

namespace st {
enum : int {
  WAVES = STATS_WAVES,
  SX = 256,  // [16][16]: 12 features, then the gradient kernel's bias column (unused here)
  LDS_FLOATS = mf::WEND + WAVES * SX
};
static_assert((size_t)LDS_FLOATS * 4 >= (size_t)WAVES * STATS_FIELDS_LS * 64 * 8, "the fold's images fit");
static_assert(LDS_FLOATS * 4 <= 64 * 1024, "static LDS");
}  // namespace st

DEV float st_lrelu(float z) { return __builtin_fmaxf(0.2f * z, z); }  // (mf_lrelu)
DEV void st_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the [16][16] SX tile's addressing (wk_ppo_mfma.hip sx): columns XOR-swizzled by 2 (row >> 1)
DEV int st_sx(int row, int col) { return row * 16 + (col ^ ((row >> 1) << 1)); }
DEV f4 st_mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// (two waves per SIMD: a full grid is two blocks per CU, and the second wave fills the first's
// MFMA dependency waits; biases and output rows are read from LDS where they are used, so the
// 256 registers hold)
// LS: the log-std pass (wk_stats.h) -- the same forward, grid and chunk ownership; the entry's
// extra arithmetic, two more double sums per lane and two more words in the block's record.
// The two instantiations are the kernels k_ppo_stats (<false>, as it always was) and
// k_ppo_logstd (<true>) below.
template <bool LS>
DEV void ppo_stats_pass(const StatsArgs& sa) {
  using namespace mf;
  using namespace st;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const GradArgs& ga = sa.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, g = lane >> 4;

  const int nchunks = (ga.samples + 15) / 16;
  const int nw = gridDim.x * WAVES;
  struct Smp { f4 sv; float act, lpo, ret, adv; };
  auto gather = [&](int c) {
    Smp m;
    const int pos = c * 16 + n;
    const size_t idx = (size_t)(pos < ga.samples ? pos : 0);
    m.sv = f4{1.0f, 0.0f, 0.0f, 0.0f};
    if (g < 3) m.sv = *(const f4*)(ga.states + idx * 12 + 4 * g);
    m.act = ga.actions[idx * 4 + g];
    m.lpo = ga.logp_old[idx * 4 + g];
    m.ret = ga.returns[idx];
    m.adv = ga.adv[idx];
    return m;
  };
  int c = blockIdx.x * WAVES + wave;
  // the first chunk's rows are in flight while the weights are staged
  Smp nxt = gather(c < nchunks ? c : 0);

  {  // the weight image, every thread's loads issued before its first LDS write
    constexpr int NV = WEND / 4, PER = (NV + 64 * WAVES - 1) / (64 * WAVES);
    f4 wv[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int e = tid + i * 64 * WAVES;
      if (e < NV) wv[i] = ((const f4*)ga.Wz)[e];
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int e = tid + i * 64 * WAVES;
      if (e < NV) ((f4*)lds)[e] = wv[i];
    }
  }
  float* cb = lds + WEND + wave * SX;
  __syncthreads();

  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const float b3g = lds[BA3 + g], bc2 = lds[BC2];
  // per-lane constants: this lane's rows of W1 / Wc1 (A operands)
  float wa1[4][3], wc1[4][3];
#pragma unroll
  for (int Mt = 0; Mt < 4; Mt++)
#pragma unroll
    for (int t = 0; t < 3; t++) {
      wa1[Mt][t] = lds[AW1F + (Mt * 3 + t) * 64 + lane];
      wc1[Mt][t] = lds[CW1F + (Mt * 3 + t) * 64 + lane];
    }
  StatsAcc<LS> acc;
#pragma unroll 1
  for (; c < nchunks; c += nw) {
    const Smp cur = nxt;
    if (c + nw < nchunks) nxt = gather(c + nw);
    const int pos = c * 16 + n;
    const bool valid = pos < ga.samples;
    {
      const int h = (n >> 1) << 1;
      const f4 v = (h & 2) ? f4{cur.sv[2], cur.sv[3], cur.sv[0], cur.sv[1]} : cur.sv;
      *(f4*)(cb + n * 16 + ((4 * g) ^ (h & 12))) = v;
    }
    st_wave_sync();
    // ---- layer 1, actor and critic ----
    float sB[3];
#pragma unroll
    for (int t = 0; t < 3; t++) sB[t] = cb[st_sx(n, 4 * t + g)];
    st_wave_sync();  // the tile is read: the next chunk may rewrite it
    f4 z1[4], zc1[4], h1[4], hc1[4];
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) { z1[Mt] = z4; zc1[Mt] = z4; }
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
      for (int Mt = 0; Mt < 4; Mt++) {
        z1[Mt] = st_mfma(wa1[Mt][t], sB[t], z1[Mt]);
        zc1[Mt] = st_mfma(wc1[Mt][t], sB[t], zc1[Mt]);
      }
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      const f4 ba1 = *(const f4*)(lds + BA1 + 16 * Mt + 4 * g);
      const f4 bc1 = *(const f4*)(lds + BC1 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        z1[Mt][r] = z1[Mt][r] + ba1[r];
        zc1[Mt][r] = zc1[Mt][r] + bc1[r];
        h1[Mt][r] = st_lrelu(z1[Mt][r]);
        hc1[Mt][r] = st_lrelu(zc1[Mt][r]);
      }
    }
    // ---- layer 2 (B operand = layer 1's D registers) ----
    f4 w2[4][4];
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++)
#pragma unroll
      for (int Mp = 0; Mp < 4; Mp++) w2[Mt][Mp] = *(const f4*)(lds + W2F + ((Mt * 4 + Mp) * 64 + lane) * 4);
    f4 z2[4], h2[4];
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) z2[Mt] = z4;
#pragma unroll
    for (int Mp = 0; Mp < 4; Mp++)
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int Mt = 0; Mt < 4; Mt++) z2[Mt] = st_mfma(w2[Mt][Mp][r], h1[Mp][r], z2[Mt]);
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      const f4 ba2 = *(const f4*)(lds + BA2 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        z2[Mt][r] = z2[Mt][r] + ba2[r];
        h2[Mt][r] = st_lrelu(z2[Mt][r]);
      }
    }
    // ---- output rows: actor z3[0..3] on h2, critic V on hc1 ----
    float p3[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pv = 0.0f;
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      const f4 wc2 = *(const f4*)(lds + WC2 + 16 * Mt + 4 * g);
      f4 w3[4];
#pragma unroll
      for (int d = 0; d < 4; d++) w3[d] = *(const f4*)(lds + W3 + d * 64 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int d = 0; d < 4; d++) p3[d] = p3[d] + w3[d][r] * h2[Mt][r];
        pv = pv + wc2[r] * hc1[Mt][r];
      }
    }
    pv = rows_sum4(pv);
    const float z3 = rows_rsum4(p3) + b3g;  // (lane (n, g): dim g)
    const float V = pv + bc2;
    const float mean = tanhf(z3);
    const float lp = stats_entry(acc, ga, valid, g == 0, mean, V, cur.act, cur.lpo, cur.ret, cur.adv);
    if (valid) {
      if (sa.logp_new) sa.logp_new[(size_t)pos * 4 + g] = lp;
      if (sa.values_new && g == 0) sa.values_new[pos] = V;
    }
  }

  // ---- lanes in lane order, waves in wave order, one record per block ----
  __syncthreads();  // every wave is done with the weights and tiles
  constexpr int NF = stats_fields<LS>();
  unsigned long long* rec = (unsigned long long*)lds;
  stats_put(acc, rec + (size_t)wave * NF * 64, lane);
  __syncthreads();
  stats_block_fold<WAVES, NF>(rec, tid, sa.partial + (size_t)blockIdx.x * NF);
}

__global__ __launch_bounds__(64 * st::WAVES) __attribute__((amdgpu_waves_per_eu(2)))
void k_ppo_stats(StatsArgs sa) { ppo_stats_pass<false>(sa); }
__global__ __launch_bounds__(64 * st::WAVES) __attribute__((amdgpu_waves_per_eu(2)))
void k_ppo_logstd(StatsArgs sa) { ppo_stats_pass<true>(sa); }

// the blocks' records in block order: sums, counts and the maximum, nothing else (the host
// divides); one block, thread f owns field f of records `nfields` words wide
__global__ __launch_bounds__(64) void k_stats_finish(const unsigned long long* __restrict__ partial,
                                                     int nblocks, int nfields, unsigned long long* out) {
  const int f = threadIdx.x;
  if (f < nfields) out[f] = stats_fold(partial + f, nblocks, nfields, f);
}

int ppo_stats_blocks(int rows) {
  const int nchunks = (rows + 15) / 16;
  const int nb = (nchunks + STATS_WAVES - 1) / STATS_WAVES;
  return nb < 1 ? 1 : (nb > STATS_MAX_BLOCKS ? (int)STATS_MAX_BLOCKS : nb);
}

hipError_t launch_ppo_stats(const StatsArgs& a, int nblocks, bool log_std, hipStream_t s) {
  hipLaunchKernelGGL(log_std ? k_ppo_logstd : k_ppo_stats, dim3(nblocks), dim3(64 * st::WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stats_finish(const unsigned long long* partial, int nblocks, bool log_std, void* out,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_stats_finish, dim3(1), dim3(64), 0, s, partial, nblocks,
                     log_std ? (int)STATS_FIELDS_LS : (int)STATS_FIELDS, (unsigned long long*)out);
  return hipGetLastError();
}

}  // namespace wk
