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
  __shared__ double sh_s1[RNORM_TILE], sh_s2[RNORM_TILE];
  __shared__ long long sh_cnt[RNORM_TILE], sh_bad[RNORM_TILE];
  long long cnt = 0, bad = 0;
  double s1 = 0.0, s2 = 0.0;
  // lane i takes tiles i, i + TILE, ... in that order, then the tree over the lanes
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
  if (tid != 0) return;
  const long long cnt_b = sh_cnt[0];
  long long count = rec->count;
  double mean = rec->mean, m2 = rec->m2;
  if (cnt_b > 0) {
    const double nb = (double)cnt_b, na = (double)count;
    const double mean_b = sh_s1[0] / nb;
    const double m2_b = fmax(0.0, sh_s2[0] - sh_s1[0] * mean_b);
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
  rec->rows = rows; rec->clipped = 0; rec->nonfinite = sh_bad[0];
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

hipError_t launch_rnorm_pass(int n, int T, float gamma, float clip, float epsilon, bool learn,
                             const float* r, const uint8_t* done, float* acc,
                             unsigned long long* partial, RnormRec* rec, float* out, hipStream_t s) {
  if (n <= 0 || T <= 0) return hipErrorInvalidValue;
  const int ntiles = rnorm_tiles(n);
  const long long rows = (long long)n * T;
  if (learn) hipLaunchKernelGGL(k_rnorm_scan, dim3(ntiles), dim3(RNORM_TILE), 0, s, n, T, gamma, r, done, acc, partial);
  hipLaunchKernelGGL(k_rnorm_finish, dim3(1), dim3(RNORM_TILE), 0, s, partial, ntiles, learn ? 1 : 0,
                     epsilon, rows, rec);
  const bool aligned = (((uintptr_t)r | (uintptr_t)out) & 15) == 0;
  const long long nvec = aligned ? rows / 4 : 0;
  const long long lanes = nvec > rows - 4 * nvec ? nvec : rows - 4 * nvec;
  const long long nb = (lanes + 255) / 256;
  hipLaunchKernelGGL(k_rnorm_apply, dim3((unsigned)(nb < 1 ? 1 : (nb > 65536 ? 65536 : nb))), dim3(256), 0, s,
                     rows, nvec, clip, r, rec, out);
  return hipGetLastError();
}

hipError_t launch_rnorm_reset(int n, const uint8_t* mask, float* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_rnorm_reset, dim3((n + 255) / 256), dim3(256), 0, s, n, mask, acc);
  return hipGetLastError();
}

}  // namespace wk
