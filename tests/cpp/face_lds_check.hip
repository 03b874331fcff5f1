// face_lds_check.hip -- the contact faces through the LDS column's one-word planes
// (significant_face_lds, csrc/wk_device.h) against the register form significant_face_ax, bit for
// bit: fa, fb, fmax, fdir for hashed pole-shaped hexagons and 5-vertex polygons with their
// normalised axes, and normals that are the polygons' own axes, their negations (projection ties
// between an edge's two vertices), hashed directions, signed zeros and units, and normals with a
// NaN component (no minimum: the idx < 0 rule).  On the same inputs also the two instantiations of
// contact_points_ax and of contact_points_floor (S > 0 against S = 0: count and both points), and
// the legs' park / unpark in the column's planes: half of the block's waves park their legs, the
// other half write face records meanwhile (the waves of the rollout kernel are not in step, so a
// lane's column must hold no other lane's word), then the legs come back bit for bit.
// One 256-thread block per launch (the rollout kernel's block, S = 256), 4 launches of 1,024
// cases per thread: 1,048,576 cases.
// Built by ppo-bipedalwalker_amd/Makefile (target `check`), run by tests/test_gpu_copy_cuts.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "wk_device.h"

using namespace wk;

constexpr int S = 256;       // the block's lanes: the planes' stride
constexpr int NCHECK = 6;    // face N = 6, face N = 5, contacts, floor contacts N = 6 / 5, park
constexpr uint32_t ITERS = 1024, LAUNCHES = 4;

__device__ uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
struct Rng {
  uint32_t s;
  __device__ uint32_t next() { s = mix(s + 0x9e3779b9u); return s; }
  __device__ float u01() { return (float)(next() >> 8) * 0x1p-24f; }
};

__device__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ bool same(V2 a, V2 b) { return same(a.x, b.x) && same(a.y, b.y); }

// a walker pole (Pole.FromSize: half width 7.5, half height 26.25) turned and moved
__device__ Poly<6> hashed_pole(Rng& r) {
  const float tx[6] = {7.5f, 0.0f, -7.5f, -7.5f, 0.0f, 7.5f};
  const float ty[6] = {26.25f, 26.25f, 26.25f, -26.25f, -26.25f, -26.25f};
  const float th = (r.u01() * 2.0f - 1.0f) * 3.14159265f;
  const float c = cosf(th), s = sinf(th);
  Poly<6> p;
  p.cx = r.u01() * 1000.0f;
  p.cy = 880.0f + r.u01() * 60.0f;  // around the floor's top edge (y = 900)
  for (int i = 0; i < 6; i++) {
    p.x[i] = tx[i] * c - ty[i] * s + p.cx;
    p.y[i] = tx[i] * s + ty[i] * c + p.cy;
  }
  return p;
}
__device__ Poly<5> hashed_pentagon(Rng& r) {
  Poly<5> p;
  p.cx = r.u01() * 1000.0f;
  p.cy = 880.0f + r.u01() * 60.0f;
  const float th0 = r.u01() * 6.2831853f;
  for (int i = 0; i < 5; i++) {
    const float th = th0 + 1.2566371f * ((float)i + 0.5f * r.u01());
    const float rad = 20.0f + 20.0f * r.u01();
    p.x[i] = rad * cosf(th) + p.cx;
    p.y[i] = rad * sinf(th) + p.cy;
  }
  return p;
}
// the SAT's normalised axes, as axis_pass forms them
template <int N>
__device__ EdgeAxes<N> axes_of(const Poly<N>& P) {
  EdgeAxes<N> a;
  for (int i = 0; i < N; i++) {
    const int i1 = (i + 1) % N;
    const V2 ax = vnormalize_edge(mk(-(P.y[i1] - P.y[i]), P.x[i1] - P.x[i]));
    a.x[i] = ax.x;
    a.y[i] = ax.y;
  }
  return a;
}
template <int NA, int NB>
__device__ V2 hashed_normal(Rng& r, const EdgeAxes<NA>& AXA, const EdgeAxes<NB>& AXB) {
  const uint32_t h = r.next();
  const uint32_t kind = h & 7u, k = (h >> 3) % 30u;
  const float special[6] = {0.0f, -0.0f, 1.0f, -1.0f, 0.70710677f, -0.70710677f};
  V2 n = mk(0.0f, 0.0f);
  for (int i = 0; i < NA; i++) if ((int)(k % NA) == i) n = mk(AXA.x[i], AXA.y[i]);
  if (kind == 2u || kind == 3u)
    for (int i = 0; i < NB; i++) if ((int)(k % NB) == i) n = mk(AXB.x[i], AXB.y[i]);
  if (kind == 1u || kind == 3u) n = vneg(n);
  if (kind == 4u || kind == 5u) {
    const float th = r.u01() * 6.2831853f;
    n = mk(cosf(th), sinf(th));
  }
  if (kind == 6u) {  // a NaN component: no projection is below MaxValue
    const float q = __uint_as_float(0x7fc00000u);
    n = (h >> 8) & 1u ? mk(q, n.y) : mk(n.x, q);
    if ((h >> 9) & 1u) n = mk(q, q);
  }
  if (kind == 7u) n = mk(special[k % 6u], special[(k / 6u) % 6u]);
  return n;
}

template <int N>
__device__ bool face_same(const Poly<N>& P, const EdgeAxes<N>& AX, V2 n, float* rec) {
  V2 a0, b0, m0, d0, a1, b1, m1, d1;
  significant_face_ax(P, AX, n, a0, b0, m0, d0);
  significant_face_lds<N, S>(P, AX, n, rec, a1, b1, m1, d1);
  __builtin_amdgcn_wave_barrier();
  return same(a0, a1) && same(b0, b1) && same(m0, m1) && same(d0, d1);
}

// out[c * S + t]: the mismatches of check c seen by thread t (vector stores only)
__global__ void __launch_bounds__(S) k_check(uint32_t seed, uint32_t* out) {
  __shared__ float col[24 * S];  // 6 records of 4 words per lane, [word][lane]
  const int t = threadIdx.x;
  float* const rec = col + t;
  Rng r{mix(seed * 0x10001u + (uint32_t)t)};
  uint32_t bad[NCHECK] = {0, 0, 0, 0, 0, 0};
  for (uint32_t it = 0; it < ITERS; it++) {
    const Poly<6> A = hashed_pole(r), B = hashed_pole(r);
    const Poly<5> T = hashed_pentagon(r);
    const EdgeAxes<6> AXA = axes_of(A), AXB = axes_of(B);
    const EdgeAxes<5> AXT = axes_of(T);
    const V2 n = hashed_normal(r, AXA, AXB);
    const V2 n5 = hashed_normal(r, AXT, AXA);
    bad[0] += !face_same(A, AXA, n, rec);
    bad[1] += !face_same(T, AXT, n5, rec);
    {
      V2 c0 = mk(0.0f, 0.0f), c1 = c0, e0 = c0, e1 = c0;
      const int k0 = contact_points_ax<6, 6, 0>(A, AXA, B, AXB, n, c0, c1);
      const int k1 = contact_points_ax<6, 6, S>(A, AXA, B, AXB, n, e0, e1, rec);
      __builtin_amdgcn_wave_barrier();
      bad[2] += !(k0 == k1 && same(c0, e0) && same(c1, e1));
    }
    {
      V2 c0 = mk(0.0f, 0.0f), c1 = c0, e0 = c0, e1 = c0;
      const int k0 = contact_points_floor<6, 0>(A, AXA, n, c0, c1);
      const int k1 = contact_points_floor<6, S>(A, AXA, n, e0, e1, rec);
      __builtin_amdgcn_wave_barrier();
      bad[3] += !(k0 == k1 && same(c0, e0) && same(c1, e1));
    }
    {
      V2 c0 = mk(0.0f, 0.0f), c1 = c0, e0 = c0, e1 = c0;
      const int k0 = contact_points_floor<5, 0>(T, AXT, n5, c0, c1);
      const int k1 = contact_points_floor<5, S>(T, AXT, n5, e0, e1, rec);
      __builtin_amdgcn_wave_barrier();
      bad[4] += !(k0 == k1 && same(c0, e0) && same(c1, e1));
    }
    // park / unpark: the waves of one parity park A and B while the others write face records
    const bool parker = (((uint32_t)t >> 6) & 1u) == (it & 1u);
    __syncthreads();
    if (parker) park_legs_planes<S>(A, B, rec);
    __syncthreads();
    V2 fa, fb, fm, fd;
    if (!parker) significant_face_lds<6, S>(B, AXB, n, rec, fa, fb, fm, fd);
    __syncthreads();
    if (parker) {
      Poly<6> lo, up;
      unpark_legs_planes<S>(lo, up, rec);
      bool ok = true;
      for (int i = 0; i < 6; i++)
        ok = ok && same(lo.x[i], A.x[i]) && same(lo.y[i], A.y[i]) && same(up.x[i], B.x[i]) &&
             same(up.y[i], B.y[i]);
      bad[5] += !ok;
    }
    __syncthreads();
  }
  for (int c = 0; c < NCHECK; c++) out[c * S + t] = bad[c];
}

int main() {
  uint32_t* d_out;
  if (hipMalloc(&d_out, NCHECK * S * sizeof(uint32_t)) != hipSuccess) return 2;
  std::vector<uint32_t> h(NCHECK * S);
  unsigned long long bad[NCHECK] = {0, 0, 0, 0, 0, 0}, total = 0;
  for (uint32_t l = 0; l < LAUNCHES; l++) {
    hipLaunchKernelGGL(k_check, dim3(1), dim3(S), 0, 0, 20250905u + l, d_out);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    if (hipMemcpy(h.data(), d_out, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return 4;
    for (int c = 0; c < NCHECK; c++)
      for (int t = 0; t < S; t++) bad[c] += h[c * S + t];
  }
  const char* name[NCHECK] = {"face N=6", "face N=5", "contact_points_ax", "contact_points_floor N=6",
                              "contact_points_floor N=5", "park / unpark"};
  for (int c = 0; c < NCHECK; c++) {
    printf("  %-26s %llu\n", name[c], bad[c]);
    total += bad[c];
  }
  printf("face column planes, %u cases: %llu mismatches\n", LAUNCHES * ITERS * (uint32_t)S, total);
  printf(total ? "FAIL\n" : "OK\n");
  return total ? 1 : 0;
}
