// wk_tail.hip -- the minibatch tail: everything that turns the gradient kernels' block slabs into a
// weight step (gfx950; the device code they share is wk_tail.h).  The ordered slab reduction of the
// built-in kernels (k_grad_reduce_fused, with Adam on one GPU) and of the general networks
// (k_net_reduce), the IPC exchange fused with both (k_reduce_xch_adam), plain Adam (k_adam) and
// gradient-norm clipping with Adam (k_clip_adam).  Built with the default flags.
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_tail.h"

namespace wk {

#define DEV __device__ __forceinline__

// Deterministic two-level sum of the block slabs in one launch (fixed association, no atomics:
// RG consecutive slabs in order, then the groups in order), for up to GRAD_MAX_BLOCKS slabs: a
// block is one job of wk_tail.h's reduce_job (QB parameter quads; thread (group gi, quad qi)
// folds its group's RG slabs with 16-byte loads, all issued before the ordered adds -- one memory
// latency, not RG -- and the 16 group sums are folded in order through LDS).  ADAM: the
// single-GPU tail applies Adam as well.  (k_reduce_xch_adam below restates the two stages.)
template <bool ADAM>
__global__ __launch_bounds__(RG * QB) void k_grad_reduce_fused(const float* __restrict__ partial,
                                                              int nblocks, float* grad, AdamArgs a) {
  static_assert(SLAB % 4 == 0 && RG * QB == 256, "16-byte slab rows, 256-thread jobs");
  __shared__ float4 gs[RG * QB];
  reduce_job<ADAM>(blockIdx.x, threadIdx.x, partial, nblocks, grad, a, gs);
}

// The general networks' slabs in block order (groups of RG consecutive slabs, then the groups:
// wk_tail.h's association) and, with a.W set, DenseLayer.Adam (DenseLayer.cs:125-159) on the np
// parameters
__global__ void k_net_reduce(const float* __restrict__ partial, int nblocks, int slabn, int np,
                             float* grad, AdamArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= slabn) return;
  const bool adam = a.W != nullptr && p < np;
  float m0 = 0.0f, v0 = 0.0f, w0 = 0.0f;
  if (adam) { m0 = a.m[p]; v0 = a.v[p]; w0 = a.W[p]; }
  float sum = 0.0f;
#pragma unroll 1
  for (int b0 = 0; b0 < nblocks; b0 += RG) {
    float v[RG];
#pragma unroll
    for (int j = 0; j < RG; j++) v[j] = (b0 + j < nblocks) ? partial[(size_t)(b0 + j) * slabn + p] : 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < RG; j++)
      if (b0 + j < nblocks) acc = acc + v[j];
    sum = sum + acc;
  }
  grad[p] = sum;
  if (adam) adam_apply(a, p, sum, m0, v0, w0);
}

// One-shot exchange (wk_comm_init_ipc): the minibatch's gradient all-reduce without a
// collective library, fused with the ordered block reduction and Adam -- one launch per
// minibatch after the gradient kernel, as on one GPU.  Block b (the grid of k_grad_reduce_fused)
// first forms this rank's ordered sum of its parameter quads exactly as k_grad_reduce_fused
// does, publishes it into this rank's exchange region (slab buffer seq & 1) and releases its
// sequence flag at system scope; it then waits (bounded) until every peer's flag b reaches
// seq, reads the peers' values directly through the IPC mappings and sums the ranks in rank
// order (rank 0's value first: for two ranks exactly the RCCL / host all-reduce's a + b), and
// applies Adam.  A buffer is reused two minibatches later only: a rank publishes seq + 2 after
// its exchange of seq + 1 saw every peer's seq + 1 flag, which a peer sets only once its own
// exchange of seq -- the last read of the seq buffers -- has completed (stream order).
// Failure: the wait is bounded by x.timeout_ticks of the constant 100 MHz clock (30 s unless
// WK_XCH_TIMEOUT_S / wk_comm_set_timeout say otherwise; ranks must stay within it of each other).
// A block whose wait times out, or that finds a peer's flag at XCH_ABORT, sets err[0], overwrites
// its own flag with XCH_ABORT and returns without writing grad_out or applying Adam; every later
// exchange sees err[0] at entry, writes XCH_ABORT into its flag and returns, so a late peer fails
// at once on that minibatch (it reads the abort value instead of this rank's sequence number)
// rather than applying it.  Block 0 records the last Adam step it applied in err[1], so the host
// rolls its step count back.  Not a consensus protocol: a peer that read this rank's sequence
// number before the abort overwrote it (a wait that ended within the same few microseconds), or
// blocks of one rank that straddle the timeout, leave the replicas' W / m / v differing -- after
// WK_ERR_COMM the job must stop or reload a checkpoint on every rank.
// Hand-off (round 6, MI355X_MICROARCH.md's valid forms at system scope): producer -- every wave's
// slab stores drained (s_waitcnt vmcnt(0)), block barrier, one lane's release store of the flag;
// consumer -- relaxed polls of the peers' flags by the polling wave, ONE acquire by that wave,
// s_waitcnt, block barrier, then the peer loads.  Adam's and grad_out's stores are written through
// (st_f<true>), so the next minibatch's release finds no dirty lines of them to write back.
// Measured uncontended at the 8-GPU shard's minibatch (profiles/r06_xch_own_*_kernel_stats.csv,
// 2 ranks on one GPU): 19.0 -> 8.2 us per launch (kernel trace), own work 13.9 -> 4.8 us per block
// (stamps), against 4.9 us for k_grad_reduce_fused<true> on the same slabs; before, every poll was
// an acquire load and every thread fenced.
// Timing (x.stamps, wk_comm_xch_profile): thread 0 reads the constant clock at entry, after its
// flag store, after the block's wait and after the block's last Adam store, and writes the four
// values with vector stores to the launch's ring slot -- wait time versus own work per minibatch.
__global__ __launch_bounds__(RG * QB) void k_reduce_xch_adam(XchArgs x) {
  __shared__ float4 gs[RG][QB];
  __shared__ int live;  // no exchange has timed out (entry), and this block's wait completed
  uint64_t ts[XCH_POINTS] = {0, 0, 0, 0};
  const bool stamp = x.stamps != nullptr && threadIdx.x == 0;
  if (stamp) ts[0] = __builtin_amdgcn_s_memrealtime();
  auto flush = [&]() {
    if (stamp)
      for (int k = 0; k < XCH_POINTS; k++) x.stamps[blockIdx.x * XCH_POINTS + k] = ts[k];
  };
  if (threadIdx.x == 0)
    live = __hip_atomic_load(x.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u ? 1 : 0;
  const int qi = threadIdx.x % QB, gi = threadIdx.x / QB;
  const int q = blockIdx.x * QB + qi;
  const int ngroups = (x.nblocks + RG - 1) / RG;
  const int p = 4 * q + gi;  // (gi < 4) this thread's parameter
  const bool adam_lane = gi < 4 && p < NPARAM && x.a.W != nullptr;  // (no W: exchange only)
  float m0 = 0.0f, v0 = 0.0f, w0 = 0.0f;
  if (adam_lane) { m0 = x.a.m[p]; v0 = x.a.v[p]; w0 = x.a.W[p]; }
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (q < SLAB / 4 && gi < ngroups) {  // stage 1, as k_grad_reduce_fused (wk_tail.h's reduce_job)
    const int b0 = gi * RG;
    float4 v[RG];
#pragma unroll
    for (int j = 0; j < RG; j++)
      v[j] = (b0 + j < x.nblocks) ? ((const float4*)(x.partial + (size_t)(b0 + j) * SLAB))[q]
                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < RG; j++)
      if (b0 + j < x.nblocks) {
        acc.x = acc.x + v[j].x; acc.y = acc.y + v[j].y;
        acc.z = acc.z + v[j].z; acc.w = acc.w + v[j].w;
      }
  }
  gs[gi][qi] = acc;
  __syncthreads();
  const int t = threadIdx.x;
  if (!live) {  // an earlier exchange failed (block-uniform: read after the barrier)
    if (t == 0)
      __hip_atomic_store(x.flag[x.rank] + blockIdx.x, XCH_ABORT, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    flush();
    return;
  }
  const int buf = (int)(x.seq & 1u);
  float mine = 0.0f;
  if (gi < 4 && q < SLAB / 4) {  // stage 2: this rank's ordered sum, published
    const float* gf = (const float*)gs;
    float gv[RG];
#pragma unroll
    for (int g = 0; g < RG; g++) gv[g] = gf[(g * QB + qi) * 4 + gi];
#pragma unroll
    for (int g = 0; g < RG; g++)
      if (g < ngroups) mine = mine + gv[g];
    x.slab[x.rank][(size_t)buf * SLAB + p] = mine;
  }
  // every storing wave drains its slab stores before the barrier: the flag's system-scope
  // release below (buffer_wbl2 in thread 0's wave) writes back only what has reached the L2 by
  // then, and a peer GPU reads this HBM over xGMI (MI355X_MICROARCH.md, inter-workgroup
  // visibility: the workgroup barrier alone does not wait for other waves' stores)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0)
    __hip_atomic_store(x.flag[x.rank] + blockIdx.x, x.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (stamp) ts[1] = __builtin_amdgcn_s_memrealtime();
  if (t < x.nranks && t != x.rank) {
    const uint64_t* f = x.flag[t] + blockIdx.x;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t seen;
    while ((seen = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) < x.seq) {
      if (__builtin_amdgcn_s_memrealtime() - t0 > x.timeout_ticks) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (seen < x.seq || seen == XCH_ABORT) {  // a peer is gone or gave up: report, never hang
      atomicOr(x.err, 1u);
      live = 0;
    }
  }
  if (t < 64) {  // ONE acquire (system scope), by the polling wave, before the barrier
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (stamp) ts[2] = __builtin_amdgcn_s_memrealtime();
  if (!live) {  // no grad_out, no Adam; a late peer reading this flag fails this minibatch too
    if (t == 0)
      __hip_atomic_store(x.flag[x.rank] + blockIdx.x, XCH_ABORT, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    flush();
    return;
  }
  if (gi < 4 && q < SLAB / 4) {
    float sum = x.rank == 0 ? mine : x.slab[0][(size_t)buf * SLAB + p];
    for (int r = 1; r < x.nranks; r++)
      sum = sum + (r == x.rank ? mine : x.slab[r][(size_t)buf * SLAB + p]);
    st_f<true>(&x.grad_out[p], sum);  // (written through: see above)
    if (adam_lane) adam_apply<true>(x.a, p, sum, m0, v0, w0);
  }
  if (blockIdx.x == 0 && t == 0 && x.a.W != nullptr)
    __hip_atomic_store(x.err + 1, x.t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (x.stamps != nullptr) {  // (block-uniform) the exit stamp after every thread's stores issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (stamp) ts[3] = __builtin_amdgcn_s_memrealtime();
    flush();
  }
}

// elementwise over all 6149 parameters
__global__ void k_adam(AdamArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < NPARAM) adam_apply(a, p, a.grad[p], a.m[p], a.v[p], a.W[p]);
}

// MaxGradNorm > 0: per-network gradient-norm clipping, then Adam, for either kernel family
// (a.grad[0..np): critic [0, n_critic), actor [n_critic, np)).  Per network
//   norm = sqrt(sum (double)g^2), coef = MaxGradNorm / (norm + 1e-6)   (double)
//   scale = (isfinite(norm) && coef < 1) ? (float)coef : 1;  Adam takes g * scale
// (torch.nn.utils.clip_grad_norm_'s form; a non-finite norm passes the gradient as it is).
// EVERY block forms both sums over the whole gradient itself -- it sits in the L2, 24 KiB for the
// built-in networks and 280 KiB for the widest general ones -- so the launch has no inter-block
// hand-off.  The association is fixed and independent of the grid: thread t of 256 takes elements
// t, t + 256, ... of a network's segment in index order (CLIP_CB loads issued ahead of their adds:
// one memory latency per batch, not per element), a wave folds its 64 partials by the xor
// butterfly (every lane gets the same bits: the adds commute), and the four wave sums are added
// in wave order.  Thread t of block b then applies Adam to parameter 256 b + t.  One lane of
// block 0 updates the record with plain loads and stores: launches are stream-ordered.
// (Batches of 32 with the two networks' first batches and butterflies interleaved measured slower,
// 12.6 against 11.7 us per launch on the built-in networks: profiles/grad_clip.json has the latter.)
enum : int { CLIP_CB = 16 };
DEV double clip_sumsq(const float* __restrict__ g, int lo, int hi, int t) {
  double s = 0.0;
#pragma unroll 1
  for (int i0 = lo + t; i0 < hi; i0 += CLIP_CB * 256) {
    float v[CLIP_CB];
#pragma unroll
    for (int j = 0; j < CLIP_CB; j++) {
      const int i = i0 + j * 256;
      v[j] = i < hi ? g[i] : 0.0f;  // (past the end: + 0 leaves the sum as it is)
    }
#pragma unroll
    for (int j = 0; j < CLIP_CB; j++) {
      const double d = (double)v[j];
      s = s + (d * d);
    }
  }
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) s = s + __shfl_xor(s, w);
  return s;
}
DEV float clip_scale(double norm, float max_norm) {
  const double coef = (double)max_norm / (norm + 1e-6);
  return (__builtin_isfinite(norm) && coef < 1.0) ? (float)coef : 1.0f;
}
__global__ __launch_bounds__(256) void k_clip_adam(AdamArgs a, int np, int n_critic, float max_norm,
                                                   GradNormRec* rec) {
  __shared__ double ws[2][4];
  const int t = threadIdx.x, p = blockIdx.x * 256 + t;
  // the Adam operands do not depend on the norms: their loads go out first
  float g0 = 0.0f, m0 = 0.0f, v0 = 0.0f, w0 = 0.0f;
  if (p < np) { g0 = a.grad[p]; m0 = a.m[p]; v0 = a.v[p]; w0 = a.W[p]; }
  const double sc = clip_sumsq(a.grad, 0, n_critic, t);
  const double sa = clip_sumsq(a.grad, n_critic, np, t);
  if ((t & 63) == 0) { ws[0][t >> 6] = sc; ws[1][t >> 6] = sa; }
  __syncthreads();
  double norm[2];
  float scale[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const double s = ((ws[k][0] + ws[k][1]) + ws[k][2]) + ws[k][3];
    norm[k] = sqrt(s);
    scale[k] = clip_scale(norm[k], max_norm);
  }
  if (p < np) adam_apply(a, p, g0 * (p < n_critic ? scale[0] : scale[1]), m0, v0, w0);
  if (blockIdx.x == 0 && t == 0) {
    rec->steps += 1;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const bool fin = __builtin_isfinite(norm[k]);
      if (scale[k] < 1.0f) rec->clipped[k] += 1;
      if (!fin) rec->nonfinite[k] += 1;
      rec->norm_last[k] = norm[k];
      if (norm[k] > rec->norm_max[k]) rec->norm_max[k] = norm[k];  // (a NaN never compares above)
      if (fin) rec->norm_sum[k] += norm[k];
      rec->scale_last[k] = scale[k];
    }
  }
}

// ---- host side ----
// adam: the single-GPU tail's Adam in the same launch, or null (grad only)
hipError_t launch_grad_reduce(const float* partial, int nblocks, float* grad, const AdamArgs* adam,
                              hipStream_t s) {
  if (nblocks > GRAD_MAX_BLOCKS) return hipErrorInvalidValue;
  const dim3 grid((SLAB / 4 + QB - 1) / QB), block(RG * QB);
  if (adam)
    hipLaunchKernelGGL(k_grad_reduce_fused<true>, grid, block, 0, s, partial, nblocks, grad, *adam);
  else
    hipLaunchKernelGGL(k_grad_reduce_fused<false>, grid, block, 0, s, partial, nblocks, grad, AdamArgs{});
  return hipGetLastError();
}
hipError_t launch_net_reduce(const float* partial, int nblocks, int np, float* grad, const AdamArgs& a,
                             hipStream_t s) {
  const int slabn = net_slab_floats(np);
  hipLaunchKernelGGL(k_net_reduce, dim3((slabn + 255) / 256), dim3(256), 0, s, partial, nblocks, slabn,
                     np, grad, a);
  return hipGetLastError();
}
int xch_blocks() { return (SLAB / 4 + QB - 1) / QB; }
size_t xch_region_bytes() { return sizeof(float) * 2 * SLAB + sizeof(uint64_t) * XCH_FLAGS; }
hipError_t launch_reduce_xch_adam(const XchArgs& x, hipStream_t s) {
  static_assert((SLAB / 4 + QB - 1) / QB <= XCH_FLAGS, "one flag per block");
  if (x.nblocks > GRAD_MAX_BLOCKS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_reduce_xch_adam, dim3((SLAB / 4 + QB - 1) / QB), dim3(RG * QB), 0, s, x);
  return hipGetLastError();
}
hipError_t launch_adam(const AdamArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_adam, dim3((NPARAM + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_clip_adam(const AdamArgs& a, int np, int n_critic, float max_norm, GradNormRec* rec,
                            hipStream_t s) {
  if (np <= 0 || n_critic < 0 || n_critic > np || !rec) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_clip_adam, dim3((np + 255) / 256), dim3(256), 0, s, a, np, n_critic, max_norm, rec);
  return hipGetLastError();
}

}  // namespace wk
