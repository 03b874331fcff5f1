// wk_returns.hip -- returns and advantages over the recorded trajectory (gfx950): the reverse scan
// of both ReturnsMode values (k_returns, k_returns_std) and the advantage normalisation
// (k_normalize).  Built with the default flags.
#include "wk_common.h"
#include "wk_kernels.h"

namespace wk {

// returns / advantages, one lane per walker, reverse scan over the [T][n] rows; done[t] ends an
// episode at t.  The operations are written out one by one (the build does not contract them):
// tests/retref.py restates them in float32 bit for bit, as _scan(mode, ...).
//   STD = false (ReturnsMode 0, k_returns): the reference (PPOAgent.cs:175-189, 414-498), whose
//     scans start from 0 and whose nextGae stays 0 (its quirk: the chain is never carried).
//   STD = true (ReturnsMode 1, k_returns_std): the standard estimators.  The scan starts from
//     vlast[e], the critic's value of the state after the last row, the GAE chain is carried, and
//     a done step clears it too.  A done step assigns 0 -- no multiply, so a non-finite bootstrap
//     value or later row never passes an episode end.
// (The pointers are unqualified here; the kernels below keep their own __restrict__.)
template <bool STD>
__device__ __forceinline__ void returns_scan(int n, int T, int use_gae, float gamma, float lambda,
                                             const float* r, const float* v, const uint8_t* done,
                                             const float* vlast, float* ret, float* adv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float start = 0.0f;
  if constexpr (STD) start = vlast[e];
  if (!use_gae) {
    float disc = start;
    for (int t = T - 1; t >= 0; t--) {
      const size_t i = (size_t)t * n + e;
      if (done[i]) disc = 0.0f;
      disc = r[i] + (disc * gamma);
      ret[i] = disc;
      adv[i] = disc - v[i];
    }
  } else {
    float nextValue = start, nextGae = 0.0f;
    for (int t = T - 1; t >= 0; t--) {
      const size_t i = (size_t)t * n + e;
      if (done[i]) { nextValue = 0.0f; if constexpr (STD) nextGae = 0.0f; }
      const float cur = v[i];
      const float delta = r[i] + (gamma * nextValue) - cur;
      const float gae = delta + (gamma * lambda * nextGae);
      adv[i] = gae;
      ret[i] = gae + cur;
      nextValue = cur;
      if constexpr (STD) nextGae = gae;
    }
  }
}

__global__ void k_returns(int n, int T, int use_gae, float gamma, float lambda,
                          const float* __restrict__ r, const float* __restrict__ v,
                          const uint8_t* __restrict__ done, float* ret, float* adv) {
  returns_scan<false>(n, T, use_gae, gamma, lambda, r, v, done, nullptr, ret, adv);
}
__global__ void k_returns_std(int n, int T, int use_gae, float gamma, float lambda,
                              const float* __restrict__ r, const float* __restrict__ v,
                              const uint8_t* __restrict__ done, const float* __restrict__ vlast,
                              float* __restrict__ ret, float* __restrict__ adv) {
  returns_scan<true>(n, T, use_gae, gamma, lambda, r, v, done, vlast, ret, adv);
}

// Normalize (PPOAgent.cs:461-472): LINQ Average/Sum accumulate in double
__global__ void k_normalize(float* x, int n, float eps_clip) {
  __shared__ double red[1024];
  __shared__ float mean_s, std_s;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += (double)x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean_s = (float)(red[0] / (double)n);
  __syncthreads();
  const float mean = mean_s;
  double ss = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double dv = (double)(x[i] - mean);
    ss += dv * dv;
  }
  __syncthreads();
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) std_s = (float)sqrt(red[0] / (double)n);
  __syncthreads();
  const float sd = std_s;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float v = x[i] - mean;
    x[i] = v / (sd + eps_clip);
  }
}

hipError_t launch_returns(int mode, int n, int T, int use_gae, float gamma, float lambda, const float* r,
                          const float* v, const uint8_t* d, const float* vlast, float* ret, float* adv,
                          hipStream_t s) {
  const dim3 grid((n + 255) / 256), block(256);
  if (mode == 1)
    hipLaunchKernelGGL(k_returns_std, grid, block, 0, s, n, T, use_gae, gamma, lambda, r, v, d, vlast, ret, adv);
  else
    hipLaunchKernelGGL(k_returns, grid, block, 0, s, n, T, use_gae, gamma, lambda, r, v, d, ret, adv);
  return hipGetLastError();
}
hipError_t launch_normalize(float* x, int n, float eps, hipStream_t s) {
  hipLaunchKernelGGL(k_normalize, dim3(1), dim3(1024), 0, s, x, n, eps);
  return hipGetLastError();
}

}  // namespace wk
