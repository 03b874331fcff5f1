// wk_render.hip -- the frame renderer's kernel (wk_render, wk_render_device, wk_render_states;
// the image is defined in include/wk_api.h, the plan in wk_render.h).
//
// One block per (tile, view).  The block reads the view's walker record into LDS (on the rough
// floor also the walker's 11 terrain heights, regenerated with terrain_draw as wk_get_body_view
// does), then thread s builds segment s of the fixed painter's order: the world endpoints from the
// record, the floor's constants or the walker's props block, the transform to pixels, d, L2 and the
// threshold (0.25f tau tau) L2.  A segment is dropped when its L2 is not > 0 (the rule lights
// nothing then) or when its pixel box, widened by tau / 2 + 1, misses the tile; the box is trusted
// only while every endpoint coordinate is within +-65,536 px, where the rule's fp32 rounding stays
// below 0.1 px -- anything larger or non-finite is kept and decided per pixel.  The survivors are
// compacted in order (one ballot per wave) into LDS; every thread then tests its four pixels against
// them in ascending order, a covering segment replacing the colour, and stores one packed pixel per
// row.  Every pixel of every view is written exactly once.  No atomics, no scratch, no divide, no
// square root; -ffp-contract=off keeps the products and sums unfused, as tests/renderref.py has them.
#include <hip/hip_runtime.h>

#include "wk_common.h"
#include "wk_render.h"

namespace wk {

namespace {

// joint k of Walker._joints (Walker.cs:182-187): record offsets of point A's and point B's x
__device__ __forceinline__ void joint_points(int k, int* a, int* b) {
  // 0: BODY v1 - LLU v4, 1: BODY v1 - RLU v4, 2: LLU v2 - LLL v3, 3: RLU v2 - RLL v3
  const int pa = k < 2 ? BODY * BSTRIDE + 2 : (k == 2 ? LLU : RLU) * BSTRIDE + 4;
  const int pb = k == 0 ? LLU * BSTRIDE + 8 : k == 1 ? RLU * BSTRIDE + 8 : (k == 2 ? LLL : RLL) * BSTRIDE + 6;
  *a = pa; *b = pb;
}

}  // namespace

__global__ __launch_bounds__(RENDER_BLOCK) void k_render(RenderPlan R, const float* __restrict__ recs,
                                                         const int32_t* __restrict__ envs,
                                                         const int32_t* __restrict__ mat,
                                                         const float* __restrict__ props,
                                                         uint32_t* __restrict__ out) {
  __shared__ float s_rec[NSTATE];
  __shared__ float s_ter[12];
  __shared__ float s_ax[WK_RENDER_MAX_SEGMENTS], s_ay[WK_RENDER_MAX_SEGMENTS], s_dx[WK_RENDER_MAX_SEGMENTS],
      s_dy[WK_RENDER_MAX_SEGMENTS], s_l2[WK_RENDER_MAX_SEGMENTS], s_thr[WK_RENDER_MAX_SEGMENTS];
  __shared__ uint32_t s_col[WK_RENDER_MAX_SEGMENTS];
  __shared__ int s_cnt[RENDER_BLOCK / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int view = blockIdx.y;
  const int tx = (int)blockIdx.x % R.tiles_x, ty = (int)blockIdx.x / R.tiles_x;
  const int e = envs[view];
  const float* rec = recs + (size_t)(R.by_view ? view : e) * NSTATE;
  if (tid < NSTATE)
    s_rec[tid] = rec[tid];
  else if (R.rough && tid < NSTATE + 11)
    s_ter[tid - NSTATE] = 800.0f + (float)terrain_draw(R.seed, (uint32_t)(R.env_offset + e), tid - NSTATE);
  __syncthreads();

  // ---- segment `tid` of the painter's order: world endpoints, thickness class, colour
  const int s = tid;
  bool keep = false;
  float au = 0.0f, av = 0.0f, du = 0.0f, dv = 0.0f, l2 = 0.0f, thr = 0.0f;
  uint32_t col = RGBA_BLACK;
  if (s < R.n_seg) {
    float x0, y0, x1, y1;
    int tc = 0;
    if (s < R.b_marker) {  // joint squares (Renderer.DrawSquare, side 3, Renderer.cs:127-135)
      const int k = s >> 2, m = s & 3, m1 = (m + 1) & 3;
      int pa, pb;
      joint_points(k, &pa, &pb);
      const float sx = (s_rec[pa] + s_rec[pb]) * 0.5f - 1.5f;
      const float sy = (s_rec[pa + 1] + s_rec[pb + 1]) * 0.5f - 1.5f;
      x0 = (m == 1 || m == 2) ? sx + 3.0f : sx;
      y0 = m >= 2 ? sy + 3.0f : sy;
      x1 = (m1 == 1 || m1 == 2) ? sx + 3.0f : sx;
      y1 = m1 >= 2 ? sy + 3.0f : sy;
      float t = s_rec[S_TORQUE + k];
      t = t != t ? 0.0f : t;  // a NaN torque counts as 0
      t = t < -1.0f ? -1.0f : (t > 1.0f ? 1.0f : t);
      const float value = (1.0f + t) * 0.5f;
      const uint32_t r = (uint32_t)(int)(value * 255.0f + 0.5f);
      const uint32_t b = (uint32_t)(int)((1.0f - value) * 255.0f + 0.5f);
      col = render_rgba(r, 0u, b);
      tc = 1;
    } else if (s < R.b_floor) {  // the best-distance marker (Environment.cs:197-199)
      x0 = R.marker_x; y0 = 500.0f; x1 = R.marker_x; y1 = 900.0f;
      col = RGBA_LIME;
      tc = 1;
    } else if (s < R.b_walker) {  // the floor: static, White
      const int f = s - R.b_floor, m = f & 3, m1 = (m + 1) & 3;
      col = RGBA_WHITE;
      if (R.rough) {  // segment k of CreateRoughFloor (Environment.cs:230-261), as wk_get_body_view
        const int k = f >> 2;
        const float x = -50.0f + 120.0f * (float)k;
        const float xp = k == 0 ? x : x - 120.0f, xn = x + 120.0f;
        const float yp = s_ter[k], y = s_ter[k + 1];
        x0 = m == 1 ? xp : (m == 3 ? xn : x);
        y0 = m == 1 ? yp : (m == 2 ? y : 1050.0f);
        x1 = m1 == 1 ? xp : (m1 == 3 ? xn : x);
        y1 = m1 == 1 ? yp : (m1 == 2 ? y : 1050.0f);
      } else {  // (-50,1050) (-50,900) (1050,900) (1050,1050) (Environment.cs:219-223)
        x0 = m < 2 ? -50.0f : 1050.0f;
        y0 = (m == 1 || m == 2) ? 900.0f : 1050.0f;
        x1 = m1 < 2 ? -50.0f : 1050.0f;
        y1 = (m1 == 1 || m1 == 2) ? 900.0f : 1050.0f;
      }
    } else if (s < R.b_prop[0]) {  // LLL, LLU, BODY, RLL, RLU: 6, 6, 5, 6, 6 edges
      const int w = s - R.b_walker;
      const int body = w < 6 ? 0 : w < 12 ? 1 : w < 17 ? 2 : w < 23 ? 3 : 4;
      const int first = body == 0 ? 0 : body == 1 ? 6 : body == 2 ? 12 : body == 3 ? 17 : 23;
      const int nv = body == BODY ? 5 : 6;
      const int m = w - first, m1 = m + 1 == nv ? 0 : m + 1;
      const int base = body * BSTRIDE;
      x0 = s_rec[base + 2 * m]; y0 = s_rec[base + 2 * m + 1];
      x1 = s_rec[base + 2 * m1]; y1 = s_rec[base + 2 * m1 + 1];
      col = render_material_rgba(mat[e]);
    } else {  // the props in scene order: xs[nv] then ys[nv] in the walker's props block
      int k = 0;
#pragma unroll
      for (int j = 1; j < RENDER_MAX_PROPS; j++)
        if (j < R.n_props && s >= R.b_prop[j]) k = j;
      // (selects, not indexed reads: the plan stays in scalar registers)
      const auto pick = [k](const auto& a) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; };
      const int nv = pick(R.prop_nv);
      const int m = s - pick(R.b_prop), m1 = m + 1 == nv ? 0 : m + 1;
      const float* p = props + (size_t)e * R.pstride + pick(R.prop_off);
      x0 = p[m]; y0 = p[nv + m];
      x1 = p[m1]; y1 = p[nv + m1];
      col = pick(R.prop_rgba);
    }
    const float oxv = R.follow ? (s_rec[S_POS] - R.half_w) + R.ox : R.ox;
    au = (x0 - oxv) * R.scale;
    av = (y0 - R.oy) * R.scale;
    const float bu = (x1 - oxv) * R.scale;
    const float bv = (y1 - R.oy) * R.scale;
    du = bu - au;
    dv = bv - av;
    l2 = du * du + dv * dv;
    thr = (tc ? R.q[1] : R.q[0]) * l2;
    keep = l2 > 0.0f;
    const float lim = 65536.0f;
    const bool tame = fabsf(au) <= lim && fabsf(av) <= lim && fabsf(bu) <= lim && fabsf(bv) <= lim;
    if (tame) {
      const float h = tc ? R.half[1] : R.half[0];
      const float tx0 = (float)(tx * RENDER_TILE_W), ty0 = (float)(ty * RENDER_TILE_H);
      const bool miss = fmaxf(au, bu) + h < tx0 || fminf(au, bu) - h > tx0 + (float)RENDER_TILE_W ||
                        fmaxf(av, bv) + h < ty0 || fminf(av, bv) - h > ty0 + (float)RENDER_TILE_H;
      keep = keep && !miss;
    }
  }
  // ---- ordered compaction of the survivors
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) s_cnt[wave] = __popcll(mask);
  __syncthreads();
  int pos = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < RENDER_BLOCK / 64; w++) {
    const int c = s_cnt[w];
    if (w < wave) pos += c;
    total += c;
  }
  if (keep) {
    s_ax[pos] = au; s_ay[pos] = av; s_dx[pos] = du; s_dy[pos] = dv; s_l2[pos] = l2; s_thr[pos] = thr;
    s_col[pos] = col;
  }
  __syncthreads();

  // ---- four pixels per thread: column `lane` of rows wave, wave + 4, wave + 8, wave + 12
  constexpr int ROWS = RENDER_TILE_H / (RENDER_BLOCK / 64);
  const int i = tx * RENDER_TILE_W + lane;
  const int j0 = ty * RENDER_TILE_H + wave;
  const float cx = (float)i + 0.5f;
  float cy[ROWS];
  uint32_t px[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    cy[r] = (float)(j0 + r * (RENDER_BLOCK / 64)) + 0.5f;
    px[r] = RGBA_BLACK;
  }
  for (int k = 0; k < total; k++) {
    const float ax = s_ax[k], ay = s_ay[k], dx = s_dx[k], dy = s_dy[k], L2 = s_l2[k], th = s_thr[k];
    const uint32_t c = s_col[k];
    const float ex = cx - ax;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const float ey = cy[r] - ay;
      const float t = ex * dx + ey * dy;
      const float cr = ex * dy - ey * dx;
      const bool hit = t >= 0.0f && t < L2 && cr * cr < th;
      px[r] = hit ? c : px[r];
    }
  }
  if (i < R.width) {
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const int j = j0 + r * (RENDER_BLOCK / 64);
      if (j < R.height) out[((size_t)view * (size_t)R.height + (size_t)j) * (size_t)R.width + (size_t)i] = px[r];
    }
  }
}

hipError_t launch_render(const RenderPlan& p, const float* recs, const int32_t* envs, const int32_t* mat,
                         const float* props, uint32_t* out, hipStream_t s) {
  const dim3 grid((unsigned)(p.tiles_x * p.tiles_y), (unsigned)p.n_views);
  hipLaunchKernelGGL(k_render, grid, dim3(RENDER_BLOCK), 0, s, p, recs, envs, mat, props, out);
  return hipGetLastError();
}

}  // namespace wk
