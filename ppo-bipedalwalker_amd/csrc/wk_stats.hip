// wk_stats.hip -- policy statistics over the trajectory for the built-in networks (gfx950):
// k_ppo_stats, a forward-only pass of the current actor and critic over every row of the buffer
// with the per-entry statistics of wk_stats.h behind it, and k_stats_finish, the ordered sum of
// the blocks' records (both kernel families); and k_ppo_logstd, the same pass instantiated with
// the log-std's derivative (wk_log_std_gradient, the LearnLogStd step).
//
// The forward pass has k_ppo_grad_mfma's operation order (wk_ppo_mfma.hip), on the helpers the two
// share (wk_mfma_tiles.h: the weight image Wz staged into LDS once per block by stage_weights, the
// chunk gather, the SX tile, mfma / mf_lrelu): one wave per chunk of 16 rows, layer 1 and 2 on
// v_mfma_f32_16x16x4_f32 with layer 1's D registers as layer 2's B operand, the output rows as
// 64-long dots on the VALU, lane (n, g) ending with z3 of dimension g and V of row n, so a row's
// mean, log-density and value are the gradient kernel's bit for bit.  The layers themselves are
// written out here a second time: this pass reads biases and output rows from LDS where it uses
// them and stores no H tiles, the gradient kernel keeps them in registers and stores the tiles
// (DESIGN.md "One derivative").  The only LDS tile a forward
// pass needs is SX.  Rows are read in buffer order; the grid is capped (STATS_MAX_BLOCKS) and the
// waves stride over the chunks, the next chunk's rows in flight during the math.
//
// Sums: each lane keeps its sums in double across its chunks in chunk order (counts as integers),
// a wave's lanes fold in lane order, a block's waves in wave order, and k_stats_finish sums the
// blocks' records in block order.  No atomics: the same inputs give the same bytes.
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_mfma_layout.h"
#include "wk_mfma_tiles.h"
#include "wk_stats.h"

namespace wk {

#define DEV __device__ __forceinline__

namespace st {
enum : int {
  WAVES = STATS_WAVES,
  SX = 256,  // [16][16]: 12 features, then the gradient kernel's bias column (unused here)
  LDS_FLOATS = mf::WEND + WAVES * SX
};
static_assert((size_t)LDS_FLOATS * 4 >= (size_t)WAVES * STATS_FIELDS_LS * 64 * 8, "the fold's images fit");
static_assert(LDS_FLOATS * 4 <= 64 * 1024, "static LDS");
}  // namespace st

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
  auto gather = [&](int c) { return gather_chunk<false, false>(ga, c, n, g); };  // (buffer order)
  int c = blockIdx.x * WAVES + wave;
  // the first chunk's rows are in flight while the weights are staged
  Smp nxt = gather(c < nchunks ? c : 0);

  stage_weights<64 * WAVES>(ga.Wz, lds, tid);
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
    sx_put(cb, n, g, cur.sv);
    wave_sync();
    // ---- layer 1, actor and critic ----
    float sB[3];
#pragma unroll
    for (int t = 0; t < 3; t++) sB[t] = cb[sx(n, 4 * t + g)];
    wave_sync();  // the tile is read: the next chunk may rewrite it
    f4 z1[4], zc1[4], h1[4], hc1[4];
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) { z1[Mt] = z4; zc1[Mt] = z4; }
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
      for (int Mt = 0; Mt < 4; Mt++) {
        z1[Mt] = mfma(wa1[Mt][t], sB[t], z1[Mt]);
        zc1[Mt] = mfma(wc1[Mt][t], sB[t], zc1[Mt]);
      }
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      const f4 ba1 = *(const f4*)(lds + BA1 + 16 * Mt + 4 * g);
      const f4 bc1 = *(const f4*)(lds + BC1 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        z1[Mt][r] = z1[Mt][r] + ba1[r];
        zc1[Mt][r] = zc1[Mt][r] + bc1[r];
        h1[Mt][r] = mf_lrelu(z1[Mt][r]);
        hc1[Mt][r] = mf_lrelu(zc1[Mt][r]);
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
        for (int Mt = 0; Mt < 4; Mt++) z2[Mt] = mfma(w2[Mt][Mp][r], h1[Mp][r], z2[Mt]);
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      const f4 ba2 = *(const f4*)(lds + BA2 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        z2[Mt][r] = z2[Mt][r] + ba2[r];
        h2[Mt][r] = mf_lrelu(z2[Mt][r]);
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
