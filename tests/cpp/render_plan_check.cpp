// render_plan_check.cpp -- the frame renderer's host side without a device: wk_render_defaults'
// values, every argument error of wk_render / wk_render_device / wk_render_states and the plan's
// segment bookkeeping (csrc/wk_render.h).  Plain host C++ with its own main, so it can be built
// with -fsanitize=address,undefined and run as it is (tests/test_render_binding.py does).
// Prints "render_plan_check ok" and returns 0, or the failed check and 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ppo-bipedalwalker_amd/csrc/wk_render.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static int check(const wk_render_args& a, const std::vector<int32_t>& envs, int n_env, const char* expect) {
  char msg[256] = "";
  unsigned char img[4];
  const int r = wk::render_check_args(&a, envs.data(), (int)envs.size(), n_env, img, 0, nullptr, msg, sizeof msg);
  if (expect) CHECK(r == WK_ERR_ARG && strstr(msg, expect));
  else CHECK(r == WK_OK && !msg[0]);
  return r;
}

int main() {
  wk_render_args d;
  memset(&d, 0x5A, sizeof d);
  wk::render_defaults(&d);
  wk::render_defaults(nullptr);
  CHECK(d.width == 550 && d.height == 325 && d.scale == 0.5f && d.ox == -50.0f && d.oy == 400.0f);
  CHECK(d.follow == 0 && d.line_px == 1.0f && std::isnan(d.marker_x) && d.joints == 1 && d.pad == 0);
  CHECK(sizeof(wk_render_args) == 40);

  const std::vector<int32_t> one{0}, ids{3, 0, 3, 2};
  check(d, ids, 4, nullptr);
  check(d, std::vector<int32_t>(WK_RENDER_MAX_VIEWS, 1), 2, nullptr);
  check(d, std::vector<int32_t>(WK_RENDER_MAX_VIEWS + 1, 1), 2, "n_views");
  check(d, {0, 4}, 4, "envs[1] = 4");
  check(d, {-1}, 4, "envs[0] = -1");
  {
    char msg[256];
    unsigned char img[4];
    float st[WK_STATE_FLOATS] = {0};
    CHECK(wk::render_check_args(nullptr, one.data(), 1, 4, img, 0, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    CHECK(wk::render_check_args(&d, nullptr, 1, 4, img, 0, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    CHECK(wk::render_check_args(&d, one.data(), 1, 4, nullptr, 0, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    CHECK(wk::render_check_args(&d, one.data(), 1, 4, img, 1, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    CHECK(wk::render_check_args(&d, one.data(), 1, 4, img, 1, st, msg, sizeof msg) == WK_OK);
    CHECK(wk::render_check_args(&d, one.data(), 0, 4, img, 0, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    CHECK(wk::render_check_args(&d, one.data(), -3, 4, img, 0, nullptr, msg, sizeof msg) == WK_ERR_ARG);
    char tiny[8];  // a short message buffer is cut, not overrun
    CHECK(wk::render_check_args(&d, one.data(), 0, 4, img, 0, nullptr, tiny, sizeof tiny) == WK_ERR_ARG && strlen(tiny) == 7);
  }
  const float nan = NAN, inf = INFINITY;
  wk_render_args a;
  a = d; a.width = 0; check(a, one, 4, "frame");
  a = d; a.width = WK_RENDER_MAX_DIM + 1; check(a, one, 4, "frame");
  a = d; a.height = -1; check(a, one, 4, "frame");
  a = d; a.width = a.height = WK_RENDER_MAX_DIM; check(a, one, 4, nullptr);
  a = d; a.width = a.height = 1; check(a, one, 4, nullptr);
  for (float bad : {0.0f, -1.0f, nan, inf, -inf}) {
    a = d; a.scale = bad; check(a, one, 4, "scale");
    a = d; a.line_px = bad; check(a, one, 4, "line_px");
  }
  for (float bad : {nan, inf, -inf}) {
    a = d; a.ox = bad; check(a, one, 4, "ox and oy");
    a = d; a.oy = bad; check(a, one, 4, "ox and oy");
  }
  for (int bad : {-1, 2}) {
    a = d; a.follow = bad; check(a, one, 4, "follow and joints");
    a = d; a.joints = bad; check(a, one, 4, "follow and joints");
  }
  a = d; a.marker_x = inf; check(a, one, 4, nullptr);  // any marker value is allowed: it draws or it does not

  // the image's size in size_t: the largest call is 64 GiB
  a = d; a.width = a.height = WK_RENDER_MAX_DIM;
  CHECK(wk::render_image_bytes(&a, WK_RENDER_MAX_VIEWS) == (size_t)1 << 36);
  CHECK(wk::render_image_bytes(&d, 64) == (size_t)64 * 325 * 550 * 4);

  // the plan: flat floor, joints, no marker, no props
  wk::RenderPlan p;
  CHECK(wk::render_make_plan(&d, 64, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, &p) == 49);
  CHECK(p.b_marker == 16 && p.b_floor == 16 && p.b_walker == 20 && p.b_prop[0] == 49 && p.b_prop[4] == 49 && p.n_seg == 49);
  CHECK(p.tiles_x == 9 && p.tiles_y == 21 && p.n_views == 64 && p.half_w == 550.0f);
  CHECK(p.tau[0] == 1.0f && p.tau[1] == 2.0f && p.q[0] == 0.25f && p.q[1] == 1.0f && p.half[0] == 1.5f && p.half[1] == 2.0f);
  // everything at once: the rough floor, a marker, the largest scene (32 vertices in 4 props)
  a = d; a.marker_x = 300.0f; a.line_px = 2.5f; a.width = 17; a.height = 9;
  const int nv[4] = {8, 8, 8, 8}, off[4] = {0, 22, 44, 66}, stat[4] = {1, 0, 0, 0}, mat[4] = {4, 4, 1, 6};
  CHECK(wk::render_make_plan(&a, 1, 1, 4, nv, off, stat, mat, 88, &p) == 118);
  CHECK(p.b_marker == 16 && p.b_floor == 17 && p.b_walker == 57 && p.b_prop[0] == 86 && p.b_prop[3] == 110 && p.b_prop[4] == 118);
  CHECK(p.prop_rgba[0] == wk::RGBA_WHITE && p.prop_rgba[1] == wk::RGBA_SANDYBROWN && p.prop_rgba[2] == wk::RGBA_CYAN &&
        p.prop_rgba[3] == wk::RGBA_SLATEGRAY);
  CHECK(p.tiles_x == 1 && p.tiles_y == 1 && p.q[0] == 1.5625f && p.q[1] == 6.25f && p.rough == 1);
  a.joints = 0;
  CHECK(wk::render_make_plan(&a, 1, 0, 1, nv, off, stat, mat, 22, &p) == 1 + 4 + 29 + 8 && p.b_marker == 0 && p.b_floor == 1);
  // refused: a prop that would read past its walker's block, too many props, too many segments
  CHECK(wk::render_make_plan(&a, 1, 0, 1, nv, off, stat, mat, 15, &p) == -1);
  CHECK(wk::render_make_plan(&a, 1, 0, 5, nv, off, stat, mat, 88, &p) == -1);
  const int big[4] = {24, 24, 24, 24}, boff[4] = {0, 54, 108, 162};
  a.joints = 1;
  CHECK(wk::render_make_plan(&a, 1, 1, 4, big, boff, stat, mat, 216, &p) == -1);  // 16 + 1 + 40 + 29 + 96
  // the material table
  const uint32_t want[8] = {wk::RGBA_GRAY, wk::RGBA_CYAN, wk::RGBA_GRAY, wk::RGBA_WHITE, wk::RGBA_SANDYBROWN,
                            wk::RGBA_GRAY, wk::RGBA_SLATEGRAY, wk::RGBA_GRAY};
  for (int m = 0; m < 8; m++) CHECK(wk::render_material_rgba(m) == want[m]);
  if (failures) return 1;
  printf("render_plan_check ok\n");
  return 0;
}
