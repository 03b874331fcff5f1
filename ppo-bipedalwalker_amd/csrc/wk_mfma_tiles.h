// wk_mfma_tiles.h -- what the kernels on the built-in networks' weight image share
// (wk_ppo_mfma.hip: k_ppo_grad_mfma / _ws / _tp; wk_stats.hip: k_ppo_stats / k_ppo_logstd):
// the matrix-core and LDS-tile primitives, the weight staging, the chunk gather and the
// block fold of the slabs.  Device code only.
#pragma once
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_mfma_layout.h"

namespace wk {

typedef float f4 __attribute__((ext_vector_type(4)));

namespace mf {
enum : int { RS = 80 };  // row stride of a [16 samples][64] tile
}  // namespace mf

// ActivationLayer LeakyReLU(0.2) = Math.Max(0.2 z, z): z for z >= 0 (and -0: Max keeps
// the equal-valued 0.2 * -0 = -0), 0.2 z below, NaN through.  As v_max_f32(0.2 z, z) it is the
// same value for every input (0.2 z is NaN exactly when z is, has z's sign, and is the larger
// one exactly when z < 0): two instructions instead of multiply, compare and select.
__device__ __forceinline__ float mf_lrelu(float z) { return __builtin_fmaxf(0.2f * z, z); }
__device__ __forceinline__ float mf_dlrelu(float z) { return z < 0.0f ? 0.2f : 1.0f; }
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// [16 samples][RS] tile addressing, bank-conflict-free both ways (MI355X_MICROARCH §LDS):
// column groups of 4 are XOR-swizzled by row bits 1..2.  A lane (n, g) stores an f4 at
// [row n][cols c..c+3] (ds_write_b128: 8-lane groups, banks mod 32 -> the 8 rows of a group
// land on 8 distinct 16-B slots); a lane (n, g) reads [row 4t + g][col 16i + n]
// (ds_read_b32: 32-lane halves; the swizzle is uniform over a half, so RS = 80 keeps the two
// rows of a half on opposite 16-bank halves).
__device__ __forceinline__ int tw(int row, int col4) { return row * mf::RS + (col4 ^ (((row >> 1) & 3) << 2)); }
__device__ __forceinline__ int tr(int row, int col) { return row * mf::RS + (col ^ (((row >> 1) & 3) << 2)); }
// [16][16] tiles (SX, G3): columns XOR-swizzled by 2 (row >> 1), read as [row n][col 4t + g]
// and [row 4t + g][col n] without conflicts; the f4 store of SX (sx_put) moves its group and
// swaps its element pairs accordingly
__device__ __forceinline__ int sx(int row, int col) { return row * 16 + (col ^ ((row >> 1) << 1)); }
__device__ __forceinline__ void sx_put(float* tile, int n, int g, f4 sv) {
  const int h = (n >> 1) << 1;
  const f4 v = (h & 2) ? f4{sv[2], sv[3], sv[0], sv[1]} : sv;
  *(f4*)(tile + n * 16 + ((4 * g) ^ (h & 12))) = v;
}
__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// sum over the 16 lanes of a DPP row (all lanes get the total)
__device__ __forceinline__ float row_sum16(float v) {
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

// Block slabs of the ordered reduction, written through to memory (sc1 buffer stores): the
// kernel-end release then has no dirty slab lines to write back out of the L2, and the
// reduction reads them from other XCDs anyway (tile-parallel kernel 12.9 -> 12.2 us per launch
// at 8,192 samples, the reduction unchanged).
struct SlabOut {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ explicit SlabOut(float* base)
      : r(__builtin_amdgcn_make_buffer_rsrc(base, 0, SLAB * 4, 0x00020000)) {}
  __device__ __forceinline__ void put(int i, f4 v) const {  // 16-byte element i
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, i * 16, 0, 16);
  }
};

// The weight image (already in operand order, wk_mfma_layout.h) into LDS by THREADS threads
// (tid < THREADS): every thread's loads are issued before its first LDS write, so the copy
// costs one L2 round trip instead of one per 4 KB.
template <int THREADS>
__device__ __forceinline__ void stage_weights(const float* Wz, float* lds, int tid) {
  constexpr int NV = mf::WEND / 4, PER = (NV + THREADS - 1) / THREADS;
  f4 wv[PER];
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int e = tid + i * THREADS;
    if (e < NV) wv[i] = ((const f4*)Wz)[e];
  }
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int e = tid + i * THREADS;
    if (e < NV) ((f4*)lds)[e] = wv[i];
  }
}

// One chunk's rows in lane (n, g): features 4 g .. 4 g + 3 of row n (lane group 3: the bias
// column {1, 0, 0, 0}), the row's action and old log-density of dimension g, its return and
// advantage.  PERM: the minibatch's rows (CreateBatches, PPOAgent.cs:512-533: base + position,
// through the permutation); otherwise the buffer's rows in order.  OPAQUE: the lane group goes
// through an opaque copy -- hoisted, `states + 4 g` was a per-lane 64-bit base that
// k_ppo_grad_ws's allocation kept in scratch and reloaded before every chunk's gather.
struct Smp { f4 sv; float act, lpo, ret, adv; };
template <bool PERM, bool OPAQUE>
__device__ __forceinline__ Smp gather_chunk(const GradArgs& ga, int c, int n, int g) {
  Smp m;
  const int pos = c * 16 + n;
  const int p0 = pos < ga.samples ? pos : 0;
  size_t idx = (size_t)p0;
  if constexpr (PERM) {
    uint32_t i = ga.base + (uint32_t)p0;
    if (ga.use_perm) i = perm_apply(i, ga.pk);
    idx = i;
  }
  uint32_t go = (uint32_t)g;
  if constexpr (OPAQUE) asm volatile("" : "+v"(go));
  m.sv = f4{1.0f, 0.0f, 0.0f, 0.0f};
  if (g < 3) m.sv = *(const f4*)(ga.states + (idx * 12 + 4 * go));
  m.act = ga.actions[idx * 4 + go];
  m.lpo = ga.logp_old[idx * 4 + go];
  m.ret = ga.returns[idx];
  m.adv = ga.adv[idx];
  return m;
}

// The block fold of N slabs at the start of LDS, after a block barrier: 16 bytes per lane and
// step with every LDS read of a lane issued up front, summed in slab order and handed to
// store(i, sum) (i: 16-byte element of the block's partial slab).  FROM_ZERO: the sum starts
// at 0 (((0 + s0) + s1) + ...), as the kernels that fold four slabs always did; otherwise at
// s0 (the two differ in the sign of a zero).
template <int THREADS, int N, bool FROM_ZERO, class Store>
__device__ __forceinline__ void fold_slabs(const float* lds, int tid, Store store) {
  const f4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  constexpr int NV = SLAB / 4, PER = (NV + THREADS - 1) / THREADS;
  f4 sv[PER][N];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int i = tid + k * THREADS;
#pragma unroll
    for (int w = 0; w < N; w++) sv[k][w] = i < NV ? ((const f4*)(lds + w * SLAB))[i] : z4;
  }
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int i = tid + k * THREADS;
    f4 acc = FROM_ZERO ? z4 + sv[k][0] : sv[k][0];
#pragma unroll
    for (int w = 1; w < N; w++) acc = acc + sv[k][w];
    if (i < NV) store(i, acc);
  }
}

}  // namespace wk
