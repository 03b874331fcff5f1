// sincos_dev_check.hip -- wk_sincos_small as the device build compiles it (csrc/wk_sincos_small.h:
// the Horner steps as three-address FMAs with scalar constants) against a plain restatement kept
// here, the same thirteen FMAs with __builtin_fma: both doubles and both (float) results bit for
// bit, for every float with |a| <= 0.25 (both signs, zeros and denormals included) and 8,192
// hashed floats outside it (any bit pattern: large values, infinities, NaNs).
// Built by ppo-bipedalwalker_amd/Makefile (target `check`), run by tests/test_gpu_copy_cuts.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "wk_sincos_small.h"

__device__ void plain_sincos_small(double x, double* s, double* c) {
  const double x2 = x * x;
  double ps = 1.0 / 6227020800.0;
  ps = __builtin_fma(ps, x2, -1.0 / 39916800.0);
  ps = __builtin_fma(ps, x2, 1.0 / 362880.0);
  ps = __builtin_fma(ps, x2, -1.0 / 5040.0);
  ps = __builtin_fma(ps, x2, 1.0 / 120.0);
  ps = __builtin_fma(ps, x2, -1.0 / 6.0);
  *s = __builtin_fma(x * x2, ps, x);
  double pc = -1.0 / 87178291200.0;
  pc = __builtin_fma(pc, x2, 1.0 / 479001600.0);
  pc = __builtin_fma(pc, x2, -1.0 / 3628800.0);
  pc = __builtin_fma(pc, x2, 1.0 / 40320.0);
  pc = __builtin_fma(pc, x2, -1.0 / 720.0);
  pc = __builtin_fma(pc, x2, 1.0 / 24.0);
  pc = __builtin_fma(pc, x2, -0.5);
  *c = __builtin_fma(x2, pc, 1.0);
}

__device__ uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

constexpr uint32_t kQuarter = 0x3e800000u;  // 0.25f: the magnitudes 0 .. 0.25 are bits 0 .. kQuarter
constexpr uint32_t kInside = 2u * (kQuarter + 1u);
constexpr uint32_t kOutside = 8192u;

// out[t]: the number of mismatching inputs seen by thread t (vector stores only)
__global__ void k_check(uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t bad = 0;
  for (uint32_t i = t; i < kInside + kOutside; i += stride) {
    uint32_t bits;
    if (i < kInside) {
      bits = (i >> 1) | ((i & 1u) << 31);
    } else {
      bits = mix(i);
      if ((bits & 0x7fffffffu) <= kQuarter) bits |= 0x40000000u;  // push it outside the range
    }
    const double x = (double)__uint_as_float(bits);
    double s0, c0, s1, c1;
    wk_sincos_small(x, &s0, &c0);
    plain_sincos_small(x, &s1, &c1);
    const bool same = __double_as_longlong(s0) == __double_as_longlong(s1) &&
                      __double_as_longlong(c0) == __double_as_longlong(c1) &&
                      __float_as_uint((float)s0) == __float_as_uint((float)s1) &&
                      __float_as_uint((float)c0) == __float_as_uint((float)c1);
    bad += !same;
  }
  out[t] = bad;
}

int main() {
  const int blocks = 2048, threads = 256, total = blocks * threads;
  uint32_t* d_out;
  if (hipMalloc(&d_out, total * sizeof(uint32_t)) != hipSuccess) return 2;
  hipLaunchKernelGGL(k_check, dim3(blocks), dim3(threads), 0, 0, d_out);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  std::vector<uint32_t> h(total);
  if (hipMemcpy(h.data(), d_out, total * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return 4;
  unsigned long long bad = 0;
  for (uint32_t v : h) bad += v;
  printf("device sincos_small, %u floats in [-0.25, 0.25] + %u outside: %llu mismatches\n", kInside,
         kOutside, bad);
  printf(bad ? "FAIL\n" : "OK\n");
  return bad ? 1 : 0;
}
