// wk_rnorm.hip -- reward normalisation (wk_reward_norm_*, gfx950): the rewards of the trajectory
// buffer scaled by the running standard deviation of the walkers' discounted returns, written to a
// second [T][n] buffer that only the returns kernels read.  Three launches:
//
//   k_rnorm_scan    one lane per walker (returns_scan's mapping, wk_returns.hip: row t of [t][e] is
//                   read coalesced), forward over t: x = r + (a * gamma) in fp32, uncontracted, as
//                   returns_scan forms r + disc * gamma; a finite x adds 1, (double)x and
//                   (double)x * (double)x (the double square of a float is exact) to the lane's
//                   count and sums and becomes the carry a, any other x is counted and zeroes the
//                   carry; a terminal row zeroes the carry; the carry goes back to acc[e].  A tile
//                   of RNORM_TILE lanes folds through LDS in a fixed tree to one partial.
//   k_rnorm_finish  one block: the tiles' partials in a fixed order, the batch's moments, Chan's
//                   merge into the running (count, mean, m2) in double, the new scale.
//   k_rnorm_apply   the streaming pass y = r * scale (one fp32 product), clamped to +-clip by
//                   copysignf (a NaN stays), float4 where the buffers are aligned; the scale is
//                   read from the device record, the clamped rows are counted with integer adds.
//
// On a record-exchange context (wk_comm_records) the finish step is split around the gather of the
// ranks' batch records: k_rnorm_batch folds the tiles' partials into this rank's record, with the
// fold k_rnorm_finish uses, and k_rnorm_merge folds the ranks' records in rank order and merges
// the result with the arithmetic k_rnorm_finish uses -- one rank gives k_rnorm_finish's bytes.
//
// No floating-point atomics: a tile's association is the tree, the tiles are summed in tile order,
// and a tile is RNORM_TILE consecutive walkers whatever the grid, so the same inputs give the
// same bytes.
#include "wk_common.h"
#include "wk_kernels.h"

namespace wk {

namespace {
// the tree over a tile's lanes: at stride s lane i takes lane i + s (s = TILE / 2 .. 1)
template <class V>
__device__ __forceinline__ void rnorm_tree(V* sh, int tid) {
#pragma unroll
  for (int s = RNORM_TILE / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    __syncthreads();
  }
}

// a batch's samples: count, non-finite count, sum x, sum x^2
struct RnormBatch {
  long long cnt, bad;
  double s1, s2;
};

// The tiles' partials folded by one block of RNORM_TILE lanes: lane i takes tiles i, i + TILE, ...
// in that order, then the tree over the lanes.  Every lane calls it and gets the result.
__device__ __forceinline__ RnormBatch rnorm_fold_tiles(const unsigned long long* __restrict__ partial,
                                                       int ntiles, int tid) {
  __shared__ double sh_s1[RNORM_TILE], sh_s2[RNORM_TILE];
  __shared__ long long sh_cnt[RNORM_TILE], sh_bad[RNORM_TILE];
  long long cnt = 0, bad = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int j = tid; j < ntiles; j += RNORM_TILE) {
    const unsigned long long* p = partial + (size_t)j * RNORM_FIELDS;
    cnt += (long long)p[0];
    bad += (long long)p[1];
    s1 += __longlong_as_double((long long)p[2]);
    s2 += __longlong_as_double((long long)p[3]);
  }
  sh_s1[tid] = s1; sh_s2[tid] = s2; sh_cnt[tid] = cnt; sh_bad[tid] = bad;
  __syncthreads();
  rnorm_tree(sh_s1, tid);
  rnorm_tree(sh_s2, tid);
  rnorm_tree(sh_cnt, tid);
  rnorm_tree(sh_bad, tid);
  return RnormBatch{sh_cnt[0], sh_bad[0], sh_s1[0], sh_s2[0]};
}

// One thread: the batch merged into the running (count, mean, m2) by Chan's formula in double, the
// new scale, and the pass's counters (`bad` the batch's non-finite samples).
__device__ __forceinline__ void rnorm_merge_store(const RnormBatch& b, float epsilon, long long rows,
                                                  RnormRec* __restrict__ rec) {
  const long long cnt_b = b.cnt;
  long long count = rec->count;
  double mean = rec->mean, m2 = rec->m2;
  if (cnt_b > 0) {
    const double nb = (double)cnt_b, na = (double)count;
    const double mean_b = b.s1 / nb;
    const double m2_b = fmax(0.0, b.s2 - b.s1 * mean_b);
    const double delta = mean_b - mean, tot = na + nb;
    mean += delta * nb / tot;
    m2 += m2_b + delta * delta * na * nb / tot;
    count += cnt_b;
  }
  const double var = count > 0 ? m2 / (double)count : 0.0;
  float scale = 1.0f;
  if (count > 0) {
    const float sc = (float)(1.0 / sqrt(var + (double)epsilon));
    if (__builtin_isfinite(sc) && sc > 0.0f) scale = sc;
  }
  rec->count = count; rec->mean = mean; rec->m2 = m2; rec->var = var;
  rec->scale = scale;
  rec->rows = rows; rec->clipped = 0; rec->nonfinite = b.bad;
}
}  // namespace

__global__ __launch_bounds__(RNORM_TILE)
void k_rnorm_scan(int n, int T, float gamma, const float* __restrict__ r,
                  const uint8_t* __restrict__ done, float* __restrict__ acc,
                  unsigned long long* __restrict__ partial) {
  __shared__ double sh_s1[RNORM_TILE], sh_s2[RNORM_TILE];
  __shared__ long long sh_cnt[RNORM_TILE], sh_bad[RNORM_TILE];
  const int tid = threadIdx.x;
  const int ntiles = (n + RNORM_TILE - 1) / RNORM_TILE;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int e = tile * RNORM_TILE + tid;
    long long cnt = 0, bad = 0;
    double s1 = 0.0, s2 = 0.0;
    if (e < n) {
      float a = acc[e];
      const auto step = [&](float rv, uint8_t dv) {
        const float x = rv + (a * gamma);
        if (__builtin_isfinite(x)) {
          const double dx = (double)x;
          cnt += 1;
          s1 += dx;
          s2 += dx * dx;
          a = x;
        } else {
          bad += 1;
          a = 0.0f;
        }
        if (dv) a = 0.0f;
      };
      int t = 0;
      // eight rows' loads in flight before the dependent chain runs over them
      for (; t + 8 <= T; t += 8) {
        float rv[8];
        uint8_t dv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const size_t i = (size_t)(t + k) * n + e;
          rv[k] = r[i];
          dv[k] = done[i];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) step(rv[k], dv[k]);
      }
      for (; t < T; t++) {
        const size_t i = (size_t)t * n + e;
        step(r[i], done[i]);
      }
      acc[e] = a;
    }
    sh_s1[tid] = s1; sh_s2[tid] = s2; sh_cnt[tid] = cnt; sh_bad[tid] = bad;
    __syncthreads();
    rnorm_tree(sh_s1, tid);
    rnorm_tree(sh_s2, tid);
    rnorm_tree(sh_cnt, tid);
    rnorm_tree(sh_bad, tid);
    if (tid == 0) {
      unsigned long long* p = partial + (size_t)tile * RNORM_FIELDS;
      p[0] = (unsigned long long)sh_cnt[0];
      p[1] = (unsigned long long)sh_bad[0];
      p[2] = (unsigned long long)__double_as_longlong(sh_s1[0]);
      p[3] = (unsigned long long)__double_as_longlong(sh_s2[0]);
    }
    __syncthreads();  // the images are read: the next tile may rewrite them
  }
}

__global__ __launch_bounds__(RNORM_TILE)
void k_rnorm_finish(const unsigned long long* __restrict__ partial, int ntiles, int learn,
                    float epsilon, long long rows, RnormRec* __restrict__ rec) {
  const int tid = threadIdx.x;
  if (!learn) {  // the apply step alone: the statistics and the scale stay as they are
    if (tid == 0) { rec->rows = rows; rec->clipped = 0; rec->nonfinite = 0; }
    return;
  }
  const RnormBatch b = rnorm_fold_tiles(partial, ntiles, tid);
  if (tid == 0) rnorm_merge_store(b, epsilon, rows, rec);
}

// this rank's batch record behind its header, the rest of the slot zero (plain vector stores)
__global__ __launch_bounds__(RNORM_TILE)
void k_rnorm_batch(const unsigned long long* __restrict__ partial, int ntiles, unsigned long long header,
                   unsigned long long* __restrict__ slot) {
  const int tid = threadIdx.x;
  const RnormBatch b = rnorm_fold_tiles(partial, ntiles, tid);
  if (tid >= RECORD_WORDS) return;
  unsigned long long w = 0ull;
  if (tid == 0) w = header;
  if (tid == 1) w = (unsigned long long)b.cnt;
  if (tid == 2) w = (unsigned long long)b.bad;
  if (tid == 3) w = (unsigned long long)__double_as_longlong(b.s1);
  if (tid == 4) w = (unsigned long long)__double_as_longlong(b.s2);
  slot[tid] = w;
}

// One thread: the ranks' batch records folded in rank order, starting from rank 0's, then
// k_rnorm_finish's merge.  Every rank runs this on the same bytes and stores the same statistics.
__global__ __launch_bounds__(64)
void k_rnorm_merge(const unsigned long long* __restrict__ all, int nranks, unsigned long long header,
                   float epsilon, long long rows, uint32_t* __restrict__ err, RnormRec* __restrict__ rec) {
  if (threadIdx.x != 0) return;
  for (int r = 0; r < nranks; r++)
    if (all[(size_t)r * RECORD_WORDS] != header) {  // a peer in another exchange: nothing is merged
      err[0] = (uint32_t)r + 1u;
      rec->rows = rows; rec->clipped = 0; rec->nonfinite = 0;
      return;
    }
  const auto rd = [&](int r) {
    const unsigned long long* p = all + (size_t)r * RECORD_WORDS + 1;
    return RnormBatch{(long long)p[0], (long long)p[1], __longlong_as_double((long long)p[2]),
                      __longlong_as_double((long long)p[3])};
  };
  RnormBatch b = rd(0);
  for (int r = 1; r < nranks; r++) {
    const RnormBatch x = rd(r);
    b.cnt += x.cnt;
    b.bad += x.bad;
    b.s1 += x.s1;
    b.s2 += x.s2;
  }
  rnorm_merge_store(b, epsilon, rows, rec);
}

// `nwords` words behind the header into a gather slot, the rest zero
__global__ __launch_bounds__(64)
void k_record_pack(const unsigned long long* __restrict__ src, int nwords, unsigned long long header,
                   unsigned long long* __restrict__ slot) {
  const int tid = threadIdx.x;
  if (tid >= RECORD_WORDS) return;
  slot[tid] = tid == 0 ? header : (tid <= nwords ? src[tid - 1] : 0ull);
}

__device__ __forceinline__ float rnorm_scaled(float r, float scale, float clip, int& clipped) {
  float y = r * scale;
  if (fabsf(y) > clip) {
    y = copysignf(clip, y);
    clipped += 1;
  }
  return y;
}

// rows [0, 4 nvec) as float4 (nvec = 0 when a buffer is not 16-byte aligned), the rest one by one
__global__ __launch_bounds__(256)
void k_rnorm_apply(long long rows, long long nvec, float clip, const float* __restrict__ r,
                   RnormRec* __restrict__ rec, float* __restrict__ out) {
  __shared__ int sh_clipped;
  if (threadIdx.x == 0) sh_clipped = 0;
  __syncthreads();
  const float scale = rec->scale;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int clipped = 0;
  for (long long i = i0; i < nvec; i += stride) {
    const float4 v = ((const float4*)r)[i];
    float4 y;
    y.x = rnorm_scaled(v.x, scale, clip, clipped);
    y.y = rnorm_scaled(v.y, scale, clip, clipped);
    y.z = rnorm_scaled(v.z, scale, clip, clipped);
    y.w = rnorm_scaled(v.w, scale, clip, clipped);
    ((float4*)out)[i] = y;
  }
  for (long long i = 4 * nvec + i0; i < rows; i += stride) out[i] = rnorm_scaled(r[i], scale, clip, clipped);
  if (clipped) atomicAdd(&sh_clipped, clipped);
  __syncthreads();
  if (threadIdx.x == 0 && sh_clipped)
    atomicAdd((unsigned long long*)&rec->clipped, (unsigned long long)sh_clipped);
}

__global__ void k_rnorm_reset(int n, const uint8_t* __restrict__ mask, float* __restrict__ acc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n && (!mask || mask[e])) acc[e] = 0.0f;
}

int rnorm_tiles(int n) { return (n + RNORM_TILE - 1) / RNORM_TILE; }

// the apply step over `rows` rewards with the scale rec holds
static void launch_rnorm_apply(long long rows, float clip, const float* r, RnormRec* rec, float* out,
                               hipStream_t s) {
  const bool aligned = (((uintptr_t)r | (uintptr_t)out) & 15) == 0;
  const long long nvec = aligned ? rows / 4 : 0;
  const long long lanes = nvec > rows - 4 * nvec ? nvec : rows - 4 * nvec;
  const long long nb = (lanes + 255) / 256;
  hipLaunchKernelGGL(k_rnorm_apply, dim3((unsigned)(nb < 1 ? 1 : (nb > 65536 ? 65536 : nb))), dim3(256), 0, s,
                     rows, nvec, clip, r, rec, out);
}

hipError_t launch_rnorm_pass(int n, int T, float gamma, float clip, float epsilon, bool learn,
                             const float* r, const uint8_t* done, float* acc,
                             unsigned long long* partial, RnormRec* rec, float* out, hipStream_t s) {
  if (n <= 0 || T <= 0) return hipErrorInvalidValue;
  const int ntiles = rnorm_tiles(n);
  const long long rows = (long long)n * T;
  if (learn) hipLaunchKernelGGL(k_rnorm_scan, dim3(ntiles), dim3(RNORM_TILE), 0, s, n, T, gamma, r, done, acc, partial);
  hipLaunchKernelGGL(k_rnorm_finish, dim3(1), dim3(RNORM_TILE), 0, s, partial, ntiles, learn ? 1 : 0,
                     epsilon, rows, rec);
  launch_rnorm_apply(rows, clip, r, rec, out, s);
  return hipGetLastError();
}

hipError_t launch_rnorm_batch(int n, int T, float gamma, const float* r, const uint8_t* done, float* acc,
                              unsigned long long* partial, unsigned long long header,
                              unsigned long long* slot, hipStream_t s) {
  if (n <= 0 || T <= 0) return hipErrorInvalidValue;
  const int ntiles = rnorm_tiles(n);
  hipLaunchKernelGGL(k_rnorm_scan, dim3(ntiles), dim3(RNORM_TILE), 0, s, n, T, gamma, r, done, acc, partial);
  hipLaunchKernelGGL(k_rnorm_batch, dim3(1), dim3(RNORM_TILE), 0, s, partial, ntiles, header, slot);
  return hipGetLastError();
}

hipError_t launch_rnorm_merge(int n, int T, float clip, float epsilon, const unsigned long long* all,
                              int nranks, unsigned long long header, uint32_t* err, const float* r,
                              RnormRec* rec, float* out, hipStream_t s) {
  if (n <= 0 || T <= 0 || nranks <= 0) return hipErrorInvalidValue;
  const long long rows = (long long)n * T;
  hipLaunchKernelGGL(k_rnorm_merge, dim3(1), dim3(64), 0, s, all, nranks, header, epsilon, rows, err, rec);
  launch_rnorm_apply(rows, clip, r, rec, out, s);
  return hipGetLastError();
}

hipError_t launch_record_pack(const void* src, int nwords, unsigned long long header,
                              unsigned long long* slot, hipStream_t s) {
  if (nwords < 0 || nwords >= RECORD_WORDS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_record_pack, dim3(1), dim3(64), 0, s, (const unsigned long long*)src, nwords, header, slot);
  return hipGetLastError();
}

hipError_t launch_rnorm_reset(int n, const uint8_t* mask, float* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_rnorm_reset, dim3((n + 255) / 256), dim3(256), 0, s, n, mask, acc);
  return hipGetLastError();
}

}  // namespace wk
