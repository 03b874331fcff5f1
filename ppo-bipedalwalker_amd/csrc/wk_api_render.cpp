// wk_api_render.cpp -- wk_render, wk_render_device, wk_render_states (kernel: wk_render.hip; the
// argument check and the plan: wk_render.h)
#include <cstring>

#include "wk_ctx.h"
#include "wk_render.h"

void wk_render_defaults(wk_render_args* a) { wk::render_defaults(a); }

// Checks, plans and launches: `states` null draws the context's records, else the host records of
// wk_render_states; the image goes to d_img.  Nothing is launched or written before every check
// has passed.  No ProfScope: the wk_profile totals stay what they were.
static int render_launch(wk_ctx* c, const wk_render_args* a, const float* states, int states_call,
                         const int32_t* envs, int n_views, const void* image, uint32_t* d_img_or_null) {
  char msg[256];
  if (wk::render_check_args(a, envs, n_views, c->n, image, states_call, states, msg, sizeof msg)) {
    c->err = msg;
    return WK_ERR_ARG;
  }
  int nv[WK_MAX_PROPS] = {0}, off[WK_MAX_PROPS] = {0}, stat[WK_MAX_PROPS] = {0}, mt[WK_MAX_PROPS] = {0};
  const int np = c->scene.n_props;
  for (int k = 0; k < np && k < WK_MAX_PROPS; k++) {
    nv[k] = c->scene.nv[k]; off[k] = c->scene.off[k]; stat[k] = c->scene.stat[k];
    mt[k] = c->scene_desc[k].material;
  }
  wk::RenderPlan p;
  if (wk::render_make_plan(a, n_views, c->P.rough, np, nv, off, stat, mt, c->scene.pstride, &p) < 0) {
    SETERR(c, "wk_render: the scene exceeds %d segments per view", (int)WK_RENDER_MAX_SEGMENTS);
    return WK_ERR_ARG;
  }
  p.seed = c->seed;
  p.env_offset = c->cfg.EnvOffset;
  p.by_view = states_call;
  uint32_t* d_img = d_img_or_null;
  if (!d_img) {
    if (ensure(c, &c->rd_img, &c->rd_img_bytes, wk::render_image_bytes(a, n_views))) return WK_ERR_HIP;
    d_img = c->rd_img;
  }
  if (ensure(c, &c->rd_envs, &c->rd_envs_bytes, sizeof(int32_t) * WK_RENDER_MAX_VIEWS)) return WK_ERR_HIP;
  // stream-ordered: an earlier render still reading the id buffer finishes first
  HIPCHK(c, hipMemcpyAsync(c->rd_envs, envs, sizeof(int32_t) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
  const float* recs = c->st;
  if (states_call) {
    const size_t bytes = sizeof(float) * wk::NSTATE * (size_t)n_views;
    if (ensure(c, &c->rd_states, &c->rd_states_bytes, bytes)) return WK_ERR_HIP;
    HIPCHK(c, hipMemcpyAsync(c->rd_states, states, bytes, hipMemcpyHostToDevice, c->stream));
    recs = c->rd_states;
  }
  HIPCHK(c, wk::launch_render(p, recs, c->rd_envs, c->mat, c->props, d_img, c->stream));
  return WK_OK;
}

// the host variants: the frames into the context's device image, then one copy and a synchronise
static int render_to_host(wk_ctx* c, const wk_render_args* a, const float* states, int states_call,
                          const int32_t* envs, int n_views, uint8_t* rgba) {
  if (int r = render_launch(c, a, states, states_call, envs, n_views, rgba, nullptr)) return r;
  HIPCHK(c, hipMemcpyAsync(rgba, c->rd_img, wk::render_image_bytes(a, n_views), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_render(wk_ctx* c, const wk_render_args* a, const int32_t* envs, int n_views, uint8_t* rgba) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  return render_to_host(c, a, nullptr, 0, envs, n_views, rgba);
}

int wk_render_device(wk_ctx* c, const wk_render_args* a, const int32_t* envs, int n_views, uint8_t* d_rgba) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (((uintptr_t)d_rgba & 3u) != 0) {
    SETERR(c, "wk_render_device: the image pointer must be 4-byte aligned (one packed store per pixel)");
    return WK_ERR_ARG;
  }
  return render_launch(c, a, nullptr, 0, envs, n_views, d_rgba, (uint32_t*)d_rgba);
}

int wk_render_states(wk_ctx* c, const wk_render_args* a, const float* states, const int32_t* envs, int n_views,
                     uint8_t* rgba) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  return render_to_host(c, a, states, 1, envs, n_views, rgba);
}
