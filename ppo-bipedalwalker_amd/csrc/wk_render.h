// wk_render.h -- what the frame renderer's host unit (wk_api_render.cpp) and device unit
// (wk_render.hip) share: the argument check, the per-call plan (the fixed painter's order as
// segment ranges, the fp32 constants of the coverage rule) and the colour table.  The check and the
// plan are plain host C++ with no device call, so a stand-alone program can run them under a
// sanitizer (tests/cpp/render_plan_check.cpp).  The image is defined in include/wk_api.h.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/wk_api.h"

namespace wk {

// a block of RENDER_BLOCK threads owns one RENDER_TILE_W x RENDER_TILE_H tile of one view: lane l
// of wave w paints column l of rows w, w + 4, w + 8, w + 12, so a wave stores whole 256-byte rows
enum : int { RENDER_TILE_W = 64, RENDER_TILE_H = 16, RENDER_BLOCK = 256, RENDER_MAX_PROPS = 4 };
static_assert(WK_RENDER_MAX_SEGMENTS <= RENDER_BLOCK, "one thread builds one segment");
static_assert(RENDER_MAX_PROPS == WK_MAX_PROPS, "prop slots");

// packed pixels: R | G << 8 | B << 16 | 255 << 24 (the bytes R, G, B, A in memory)
constexpr uint32_t render_rgba(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16 | 0xFF000000u; }
enum : uint32_t {
  RGBA_BLACK = 0xFF000000u, RGBA_WHITE = 0xFFFFFFFFu, RGBA_LIME = 0xFF00FF00u, RGBA_GRAY = 0xFF808080u,
  RGBA_CYAN = 0xFFFFFF00u, RGBA_SANDYBROWN = 0xFF60A4F4u, RGBA_SLATEGRAY = 0xFF908070u
};
static_assert(render_rgba(244, 164, 96) == RGBA_SANDYBROWN && render_rgba(112, 128, 144) == RGBA_SLATEGRAY &&
              render_rgba(0, 255, 255) == RGBA_CYAN && render_rgba(128, 128, 128) == RGBA_GRAY, "XNA colours");

// Materials/<Name>.cs GetColor(): XNA's named colours
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t render_material_rgba(int mat) {
  switch (mat) {
    case WK_MAT_ICE: return RGBA_CYAN;
    case WK_MAT_METAL: return RGBA_WHITE;
    case WK_MAT_WOOD: return RGBA_SANDYBROWN;
    case WK_MAT_TITANIUM: return RGBA_SLATEGRAY;
    default: return RGBA_GRAY;  // Carpet, Rubber, Paper, SuperRubber
  }
}

// One call's plan, passed to the kernel by value.  Segment s of a view, in painter's order:
// [0, b_marker) the joint squares' edges, [b_marker, b_floor) the marker, [b_floor, b_walker) the
// floor's edges, [b_walker, b_prop[0]) the 29 walker edges, [b_prop[k], b_prop[k + 1]) prop k's.
struct RenderPlan {
  int width, height, n_views, tiles_x, tiles_y;
  int follow, rough, by_view;  // by_view: view i reads record i (wk_render_states), else record envs[i]
  float scale, ox, oy;
  float half_w;                // follow: 0.5f * ((float)width / scale)
  float marker_x;
  float tau[2], q[2], half[2]; // [0] outlines, [1] joints and marker: thickness, 0.25f * tau * tau,
                               // and the culling box's margin 0.5f * tau + 1
  int b_marker, b_floor, b_walker, b_prop[RENDER_MAX_PROPS + 1], n_seg;
  int n_props, pstride, prop_nv[RENDER_MAX_PROPS], prop_off[RENDER_MAX_PROPS];
  uint32_t prop_rgba[RENDER_MAX_PROPS];
  int env_offset;
  uint64_t seed;
};

// wk_render_defaults: the whole flat floor and the walker in 550 x 325 pixels
inline void render_defaults(wk_render_args* a) {
  if (!a) return;
  memset(a, 0, sizeof(*a));
  a->width = 550; a->height = 325;
  a->scale = 0.5f;
  a->ox = -50.0f; a->oy = 400.0f;
  a->follow = 0;
  a->line_px = 1.0f;
  a->marker_x = std::numeric_limits<float>::quiet_NaN();
  a->joints = 1;
}

// the image's bytes, in size_t (4,096 views of 2,048 x 2,048 are 64 GiB)
inline size_t render_image_bytes(const wk_render_args* a, int n_views) {
  return (size_t)n_views * (size_t)a->height * (size_t)a->width * 4u;
}

// Every argument error of wk_render / wk_render_device / wk_render_states; 0 or WK_ERR_ARG with the
// text in msg.  `states` is checked only when states_call is set.
inline int render_check_args(const wk_render_args* a, const int32_t* envs, int n_views, int n_env,
                             const void* image, int states_call, const void* states, char* msg, size_t cap) {
#define WK_RENDER_FAIL(...) do { snprintf(msg, cap, __VA_ARGS__); return WK_ERR_ARG; } while (0)
  if (!a) WK_RENDER_FAIL("wk_render: args is NULL");
  if (!envs) WK_RENDER_FAIL("wk_render: envs is NULL");
  if (!image) WK_RENDER_FAIL("wk_render: the image pointer is NULL");
  if (states_call && !states) WK_RENDER_FAIL("wk_render_states: states is NULL");
  if (n_views < 1 || n_views > WK_RENDER_MAX_VIEWS)
    WK_RENDER_FAIL("wk_render: n_views %d outside 1..%d", n_views, (int)WK_RENDER_MAX_VIEWS);
  if (a->width < 1 || a->width > WK_RENDER_MAX_DIM || a->height < 1 || a->height > WK_RENDER_MAX_DIM)
    WK_RENDER_FAIL("wk_render: frame %d x %d outside 1..%d", a->width, a->height, (int)WK_RENDER_MAX_DIM);
  if (!(std::isfinite(a->scale) && a->scale > 0.0f)) WK_RENDER_FAIL("wk_render: scale must be finite and > 0");
  if (!(std::isfinite(a->line_px) && a->line_px > 0.0f)) WK_RENDER_FAIL("wk_render: line_px must be finite and > 0");
  if (!std::isfinite(a->ox) || !std::isfinite(a->oy)) WK_RENDER_FAIL("wk_render: ox and oy must be finite");
  if (a->follow < 0 || a->follow > 1 || a->joints < 0 || a->joints > 1)
    WK_RENDER_FAIL("wk_render: follow and joints are 0 or 1");
  for (int i = 0; i < n_views; i++)
    if (envs[i] < 0 || envs[i] >= n_env)
      WK_RENDER_FAIL("wk_render: envs[%d] = %d outside [0, %d)", i, (int)envs[i], n_env);
#undef WK_RENDER_FAIL
  return WK_OK;
}

// The plan of checked arguments on a context with the given floor and scene (prop_nv / prop_off:
// the props' vertex counts and offsets inside a walker's props block; prop_static / prop_material:
// what colours them).  Returns the segment count, at most WK_RENDER_MAX_SEGMENTS, or -1.
inline int render_make_plan(const wk_render_args* a, int n_views, int rough, int n_props, const int* prop_nv,
                            const int* prop_off, const int* prop_static, const int* prop_material,
                            int pstride, RenderPlan* p) {
  *p = RenderPlan{};
  if (n_props < 0 || n_props > RENDER_MAX_PROPS) return -1;
  p->width = a->width; p->height = a->height; p->n_views = n_views;
  p->tiles_x = (a->width + RENDER_TILE_W - 1) / RENDER_TILE_W;
  p->tiles_y = (a->height + RENDER_TILE_H - 1) / RENDER_TILE_H;
  p->follow = a->follow; p->rough = rough ? 1 : 0;
  p->scale = a->scale; p->ox = a->ox; p->oy = a->oy;
  p->half_w = 0.5f * ((float)a->width / a->scale);
  p->marker_x = a->marker_x;
  p->tau[0] = a->line_px;
  p->tau[1] = 2.0f * a->line_px;
  for (int i = 0; i < 2; i++) {
    p->q[i] = 0.25f * p->tau[i] * p->tau[i];
    p->half[i] = 0.5f * p->tau[i] + 1.0f;
  }
  int s = a->joints ? 16 : 0;
  p->b_marker = s;
  s += std::isnan(a->marker_x) ? 0 : 1;
  p->b_floor = s;
  s += rough ? 40 : 4;
  p->b_walker = s;
  s += 29;
  p->n_props = n_props; p->pstride = pstride;
  for (int k = 0; k < n_props; k++) {
    if (prop_nv[k] < 1 || prop_nv[k] > WK_PROP_MAXV) return -1;
    if (prop_off[k] < 0 || prop_off[k] + 2 * prop_nv[k] > pstride) return -1;  // xs[nv] ys[nv] inside the block
    p->b_prop[k] = s;
    p->prop_nv[k] = prop_nv[k];
    p->prop_off[k] = prop_off[k];
    p->prop_rgba[k] = prop_static[k] ? (uint32_t)RGBA_WHITE : render_material_rgba(prop_material[k]);
    s += prop_nv[k];
  }
  for (int k = n_props; k <= RENDER_MAX_PROPS; k++) p->b_prop[k] = s;
  p->n_seg = s;
  return s <= WK_RENDER_MAX_SEGMENTS ? s : -1;
}

#if defined(__HIPCC__)
// wk_render.hip: one launch paints every pixel of every view once (background included)
hipError_t launch_render(const RenderPlan& p, const float* recs, const int32_t* envs, const int32_t* mat,
                         const float* props, uint32_t* out, hipStream_t s);
#endif

}  // namespace wk
