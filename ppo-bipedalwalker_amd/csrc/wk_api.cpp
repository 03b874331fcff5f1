// wk_api.cpp -- C-ABI implementation (include/wk_api.h), the context's unit: defaults and
// validation, create / destroy / reset, the walkers' materials and offsets, weights and Adam state,
// the learning rate, profiling.  The other host units are wk_api_{env,rollout,update,comm,eval,io}.cpp;
// what they share is in wk_ctx.h.
//
// Host responsibilities only: argument validation (Hyperparameters validation,
// Walker/PPO/Hyperparameters.cs:189-217), buffer management, the per-minibatch launch
// sequence of PPOAgent.Train(Trajectory) (PPOAgent.cs:147-172) and the double-precision
// Adam bias corrections (DenseLayer.cs:142-145: (float)(1 - Math.Pow(beta, t))).
// Every compute step runs in a HIP kernel; there is no CPU fallback.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "wk_ctx.h"
#include "wk_text.h"

static const char* kCriticDefault = "Input |64| (LeakyReLU) |1| Output";
static const char* kActorDefault = "Input |64| (LeakyReLU) |64| (LeakyReLU) |4| (TanH) Output";
static thread_local std::string g_create_error;
namespace wk {
void set_last_error(const std::string& msg) { g_create_error = msg; }
}  // namespace wk

hipEvent_t ev_get(wk_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

static void prof_drain(wk_ctx* c) {
  for (auto& e : c->pending) {
    float ms = 0.0f;
    if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->prof_ms[e.kind] += ms;
      c->prof_cnt[e.kind] += 1;
      if (e.kind == PK_PHYS) c->prof_units += e.units;
    }
    c->pool.push_back(e.a);
    c->pool.push_back(e.b);
  }
  c->pending.clear();
}

void wk_config_defaults(wk_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->GameSpeed = 1;
  c->Iterations = 50;
  c->MaxTimesteps = 1000;
  c->RoughFloor = 0;
  c->Epochs = 5;
  c->BatchSize = 64;
  c->UseGAE = 0;
  c->NormalizeAdvantages = 0;
  c->Gamma = 0.9f;
  c->Lambda = 0.95f;
  c->Epsilon = 0.3f;
  c->LogStandardDeviation = -1.0f;
  c->Alpha = 0.001f;
  c->Beta1 = 0.9f;
  c->Beta2 = 0.999f;
  c->AdamEpsilon = 1e-8f;
  c->CriticNeuralNetwork = nullptr;
  c->ActorNeuralNetwork = nullptr;
  c->DeltaTime = (float)(166667.0 / 10000000.0);
  c->Horizon = 64;
  c->Minibatch = 0;
  c->MinibatchGlobal = 0;
  c->EnvOffset = 0;
  c->RandomizeStart = 0;
  c->RandomizeMaterial = 0;
  c->NetworkKernels = 0;
  c->ReturnsMode = 0;
  c->TargetKL = 0.0f;
  c->MaxGradNorm = 0.0f;
  c->LearnLogStd = 0;
  c->LogStdAlpha = 0.0f;
  c->EntropyCoef = 0.0f;
  c->LogStdMin = -4.0f;
  c->LogStdMax = 1.0f;
}

const char* wk_version(void) { return "wk 0.1 (gfx950)"; }

const char* wk_last_error(const wk_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

// ValidateHyperparameterValues (Hyperparameters.cs:189-217) + the kernel's fixed shapes
static int validate(const wk_config* c, std::string& why) {
  char b[256];
  auto bad = [&](const char* m) { why = m; return WK_ERR_CONFIG; };
  if (c->GameSpeed <= 0 || c->GameSpeed >= 10) return bad("Invalid game speed, should be in range 0<x<10");
  if (c->Iterations <= 0 || c->Iterations >= 200) return bad("Invalid iterations count, should be in range 0<x<200");
  if (c->MaxTimesteps <= 0) return bad("Invalid maximum time steps amount, should be in range x>0");
  if (c->Alpha <= 0 || c->Alpha >= 10) return bad("Invalid alpha value, should be in range 0<x<10");
  if (c->Beta1 <= 0 || c->Beta1 > 1) return bad("Invalid beta1 value, should be in range 0<x<1");
  if (c->Beta2 <= 0 || c->Beta2 > 1) return bad("Invalid beta2 value, should be in range 0<x<1");
  if (c->AdamEpsilon <= 0 || c->AdamEpsilon >= 1) return bad("Invalid Adam epsilon value, should be in range 0<x<1");
  if (c->Epochs <= 0 || c->Epochs >= 50) return bad("Invalid epochs value, should be in range 0<x<50");
  if (c->BatchSize <= 0 || c->BatchSize >= 1000) return bad("Invalid batch size value, should be in range 0<x<1000");
  if (c->Gamma <= 0 || c->Gamma > 1) return bad("Invalid gamma value, should be in range 0<x<1");
  if (c->Lambda <= 0 || c->Lambda > 1) return bad("Invalid lambda value, should be in range 0<x<1");
  if (c->Epsilon <= 0 || c->Epsilon > 1) return bad("Invalid epsilon value, should be in range 0<x<1");
  if (c->LogStandardDeviation <= -5 || c->LogStandardDeviation >= 5) return bad("Invalid log standard deviation value, should be in range -5<x<5");
  if (c->NetworkKernels != 0 && c->NetworkKernels != 1) return bad("NetworkKernels must be 0 (built-in kernels) or 1 (general kernels)");
  if (c->NetworkKernels == 0) {
    if (c->CriticNeuralNetwork && strcmp(c->CriticNeuralNetwork, kCriticDefault) != 0) {
      snprintf(b, sizeof(b), "critic network '%.60s' unsupported: the built-in kernels implement '%s' "
               "(NetworkKernels = 1 selects the general kernels)", c->CriticNeuralNetwork, kCriticDefault);
      why = b;
      return WK_ERR_CONFIG;
    }
    if (c->ActorNeuralNetwork && strcmp(c->ActorNeuralNetwork, kActorDefault) != 0) {
      snprintf(b, sizeof(b), "actor network '%.60s' unsupported: the built-in kernels implement '%s' "
               "(NetworkKernels = 1 selects the general kernels)", c->ActorNeuralNetwork, kActorDefault);
      why = b;
      return WK_ERR_CONFIG;
    }
  } else {  // the general kernels: any valid string within wk_net.h's limits
    wk::NetSpec ns;
    if (!wk::net_spec(c->CriticNeuralNetwork, c->ActorNeuralNetwork, ns, why)) return WK_ERR_CONFIG;
  }
  if (c->ReturnsMode != 0 && c->ReturnsMode != 1)
    return bad("ReturnsMode must be 0 (the reference's returns) or 1 (chained GAE, bootstrap at the cut)");
  if (!std::isfinite(c->TargetKL) || c->TargetKL < 0.0f)
    return bad("TargetKL must be finite and >= 0 (0: no early stop)");
  if (!(c->MaxGradNorm >= 0.0f))  // (a NaN compares false; +inf measures only)
    return bad("MaxGradNorm must be >= 0 and not NaN (0: no clipping, inf: measure only)");
  if (c->LearnLogStd != 0 && c->LearnLogStd != 1)
    return bad("LearnLogStd must be 0 (a constant log-std) or 1 (trained after every epoch)");
  if (!std::isfinite(c->LogStdAlpha) || c->LogStdAlpha < 0.0f)
    return bad("LogStdAlpha must be finite and >= 0 (0: the context's Alpha)");
  if (!std::isfinite(c->EntropyCoef) || c->EntropyCoef < 0.0f)
    return bad("EntropyCoef must be finite and >= 0");
  if (c->EntropyCoef > 0.0f && c->LearnLogStd == 0)
    return bad("EntropyCoef > 0 needs LearnLogStd = 1: with a fixed log-std the entropy bonus is a constant");
  if (c->LearnLogStd == 1 &&
      !(c->LogStdMin > -5.0f && c->LogStdMin <= c->LogStandardDeviation &&
        c->LogStandardDeviation <= c->LogStdMax && c->LogStdMax < 5.0f))  // (a NaN compares false)
    return bad("LearnLogStd = 1 needs -5 < LogStdMin <= LogStandardDeviation <= LogStdMax < 5");
  if (c->Horizon <= 0) return bad("Horizon must be > 0");
  if (c->Minibatch < 0) return bad("Minibatch must be >= 0");
  if (c->LanesPerWalker != 0 && c->LanesPerWalker != 1 && c->LanesPerWalker != 2 &&
      c->LanesPerWalker != 4 && c->LanesPerWalker != 16)
    return bad("LanesPerWalker must be 0 (auto), 1, 2, 4 or 16");
  return WK_OK;
}

// The rough floor's lane order (split mappings): the walkers sorted by start offset, so that a
// wave's walkers stand over the same stretch of terrain and its floor-segment loop resolves the
// union of fewer segments (Environment.cs:230-261: segments 240 px wide every 120 px; the
// offsets span 200 px).  Static -- a walker keeps its offset, and rough-floor episodes end
// within a few steps, so the flat floor's episode-0 partition has nothing to gather -- and
// recomputed whenever the offsets change (wk_create, wk_set_offsets, wk_checkpoint_load).
// Measured with the offsets themselves sorted by walker id (scripts/rough_dx_sort.py): rollout
// 110 -> 87.6 ms at 65,536 walkers (pair), 63.9 -> 50.4 ms at 8,192 (quad).  Bit-identical:
// every walker's arithmetic is keyed by its id (tests/test_gpu_order.py).
hipError_t rough_order_upload(wk_ctx* c, const float* dx_host) {
  if (!c->order || !c->P.rough || !(c->P.lanes == 2 || c->P.lanes == 4)) return hipSuccess;
  std::vector<int32_t> ord(c->n);
  for (size_t e = 0; e < c->n; e++) ord[e] = (int32_t)e;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
    return dx_host[a] < dx_host[b];  // (a NaN offset compares false: it keeps its relative place)
  });
  return hipMemcpy(c->order, ord.data(), sizeof(int32_t) * c->n, hipMemcpyHostToDevice);
}

// W in the matrix-core operand order, for the built-in gradient kernels
hipError_t upload_image(wk_ctx* c) {
  return c->general ? hipSuccess : wk::launch_swizzle(c->W, c->Wz, c->stream);
}

// the eight [T][n] trajectory rows in wk_get_trajectory's argument order, with bytes per sample
std::array<TrajRow, 8> traj_rows(wk_ctx* c) {
  const size_t f = sizeof(float);
  return {{{"ts", (void**)&c->ts, 12 * f}, {"ta", (void**)&c->ta, 4 * f}, {"tlp", (void**)&c->tlp, 4 * f},
           {"tr", (void**)&c->tr, f}, {"td", (void**)&c->td, 1}, {"tv", (void**)&c->tv, f},
           {"tret", (void**)&c->tret, f}, {"tadv", (void**)&c->tadv, f}}};
}

// The policy's log-std and everything derived from it, in one place (wk_create, wk_set_log_std,
// the LearnLogStd step, snapshot and checkpoint): every kernel takes these by value at launch
void apply_log_std(wk_ctx* c, float log_std) {
  c->P.log_std = log_std;
  c->P.std_ = expf(log_std);
  const float PI_F = 3.14159265358979323846f;
  c->lp_const = -logf(c->P.std_) - logf(sqrtf(2.0f * PI_F));
}

int wk_create(const wk_config* cfg, int device, int n_env, uint64_t seed, wk_ctx** out) {
  if (!out) { g_create_error = "out is NULL"; return WK_ERR_ARG; }
  *out = nullptr;
  wk_config c;
  if (cfg) c = *cfg; else wk_config_defaults(&c);
  if (n_env <= 0) { g_create_error = "n_env must be > 0"; return WK_ERR_ARG; }
  std::string why;
  int vs = validate(&c, why);
  if (vs != WK_OK) { g_create_error = why; return vs; }
  int ndev = 0;
  hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev == 0) {
    g_create_error = std::string("no HIP device available: ") + hipGetErrorString(he);
    return WK_ERR_HIP;
  }
  if (device < 0 || device >= ndev) { g_create_error = "device index out of range"; return WK_ERR_ARG; }
  struct Restore {  // the caller's current device, as every other entry point leaves it
    int prev = -1;
    Restore() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~Restore() { if (prev >= 0) (void)hipSetDevice(prev); }
  } restore;
  wk_ctx* x = new wk_ctx();
  x->cfg = c;
  // the strings are copied: the caller's pointers are borrowed for this call only
  x->general = c.NetworkKernels == 1;
  if (!wk::net_spec(x->general ? c.CriticNeuralNetwork : nullptr, x->general ? c.ActorNeuralNetwork : nullptr,
                    x->net, why)) {
    g_create_error = why;
    delete x;
    return WK_ERR_CONFIG;
  }
  x->cfg.CriticNeuralNetwork = x->net.critic_str.c_str();
  x->cfg.ActorNeuralNetwork = x->net.actor_str.c_str();
  x->np = x->net.np;
  x->slabn = x->general ? wk::net_slab_floats(x->np) : (int)wk::SLAB;
  x->act_rows = wk::net_act_rows(x->net.critic, x->net.actor);
  if (x->cfg.Minibatch == 0) x->cfg.Minibatch = x->cfg.BatchSize;
  x->device = device;
  x->n = n_env;
  x->seed = seed;
  x->T = c.Horizon;
  auto fail = [&](int code) {
    g_create_error = x->err;
    wk_destroy(x);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) { x->err = "hipSetDevice failed"; return fail(WK_ERR_HIP); }
  // > 64 KiB dynamic LDS for the gradient kernels, set on this device (the attribute is
  // per device; wk_create is the only place, so launches never race on it)
  if (wk::configure_device_kernels() != hipSuccess || wk::configure_net_kernels() != hipSuccess) {
    x->err = "hipFuncSetAttribute failed";
    return fail(WK_ERR_HIP);
  }
  x->grad_impl = wk::grad_impl_env();
  if (hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess) {
    x->err = "hipStreamCreate failed";
    return fail(WK_ERR_HIP);
  }
  auto& P = x->P;
  P.n_env = n_env;
  P.iterations = c.Iterations;
  P.max_timesteps = c.MaxTimesteps;
  P.dt_frame = c.DeltaTime;
  P.dt_sub = c.DeltaTime / (float)c.Iterations;
  apply_log_std(x, c.LogStandardDeviation);
  P.seed = seed;
  P.env_offset = c.EnvOffset;
  // auto on the flat floor: the side-split pair mapping from 16,385 walkers up, the quad
  // mapping (two lanes per leg) below -- measured on one MI355X (scripts/side_times.sh,
  // rollout T = 16): 5.94 vs 7.56 ms at 8,192 and 16,384 walkers (one wave per SIMD at most,
  // where the split shortens each wave's chain), 11.7 vs 7.6 ms at 32,768 (two waves per
  // SIMD: issue-bound, the split's extra selects and exchanges cost more than they save).
  // Round 1: the pair mapping 32.1 ms at 8,192 walkers vs 83.2 ms for the 16-lane rows and
  // 104 ms one lane per walker (T = 64).  The rough floor takes the same choice: its segment
  // pairs run unsplit in every mapping, the leg-leg pairs keep the pair / quad split.
  P.lanes = c.LanesPerWalker ? c.LanesPerWalker : (n_env <= 16384 ? 4 : 2);
  P.rough = c.RoughFloor ? 1 : 0;
  // the quad mapping with fewer walkers per wave (the other lanes replay them) while one wave
  // per SIMD still holds every walker (1,024 SIMDs): each wave's divergent branches are the
  // union over fewer walkers -- rollout 5.72 -> 5.52 ms per 16 env-steps at 8,192 walkers
  // (eight per wave), physics only 5.95 -> 5.62.  Test hook (tests/test_gpu_parity.py, the
  // sparse mapping against the dense one): WK_QUAD_SPARSE=0 at wk_create, always sixteen
  {
    const char* sp = getenv("WK_QUAD_SPARSE");
    int wpw = 16;
    if (!(sp && sp[0] == '0'))
      while (wpw > 1 && (size_t)n_env <= (size_t)512 * wpw) wpw >>= 1;  // n / (wpw / 2) <= 1,024 waves
    P.wpw = wpw;
  }

  const size_t n = (size_t)n_env, T = (size_t)x->T;
#define ALLOC(ptr, bytes)                                                   \
  if (dev_alloc(x, &(ptr), (bytes)) != hipSuccess) {                       \
    x->err = "hipMalloc failed for " #ptr;                                  \
    return fail(WK_ERR_HIP);                                                \
  }
  ALLOC(x->st, sizeof(float) * wk::NSTATE * n);
  ALLOC(x->dxoff, sizeof(float) * n);
  ALLOC(x->mat, sizeof(int32_t) * n);
  ALLOC(x->rng_t, sizeof(uint32_t) * n);
  const size_t np = (size_t)x->np;
  ALLOC(x->W, sizeof(float) * np);
  if (x->general) {  // (no operand-order image: the general kernels read W as it is)
    ALLOC(x->net_dev, sizeof(wk::NetDesc) * 2);
  } else {
    ALLOC(x->Wz, sizeof(float) * wk::mfma_image_floats());
  }
  ALLOC(x->m, sizeof(float) * np);
  ALLOC(x->v, sizeof(float) * np);
  ALLOC(x->grad, sizeof(float) * x->slabn);
  for (const TrajRow& r : traj_rows(x))
    if (dev_alloc(x, r.p, r.bytes * n * T) != hipSuccess) {
      x->err = std::string("hipMalloc failed for x->") + r.name;
      return fail(WK_ERR_HIP);
    }
  if (c.ReturnsMode == 1) ALLOC(x->vlast, sizeof(float) * n);
  if (c.MaxGradNorm > 0.0f) ALLOC(x->gnorm, sizeof(wk::GradNormRec));
  x->ep_cap = (uint64_t)n * T;  // one rollout's worst case: every env-step ends an episode
  x->loss_cap = 1u << 16;
  ALLOC(x->ep_acc, sizeof(double) * n);
  ALLOC(x->ep_len, sizeof(int32_t) * n);
  ALLOC(x->ep_scratch, sizeof(float) * 2 * n * T);
  ALLOC(x->ep_rowcnt, sizeof(uint32_t) * wk::episode_count_cells((int)n, T));
  ALLOC(x->ep_count, sizeof(uint64_t));
  ALLOC(x->ep_log, sizeof(wk::EpisodeRecDev) * x->ep_cap);
  ALLOC(x->loss_log, sizeof(float) * 2 * x->loss_cap);
  // test hook (tests/test_gpu_order.py, the lane order against the identity order): WK_ORDER=0
  if (P.lanes == 2 || P.lanes == 4) {
    const char* o = getenv("WK_ORDER");
    if (!(o && o[0] == '0')) {
      ALLOC(x->order, sizeof(int32_t) * 3 * n);  // order, then the swap ranks' scratch
      ALLOC(x->order_cnt, sizeof(uint32_t) * wk::order_cells((int)n));
    }
  }
  // pacing of co-resident waves (k_env_side's pair mapping, k_env_step; the quad mapping runs one
  // wave per SIMD); test hook WK_PACE=0: without
  if (P.lanes != 4) {
    const char* o = getenv("WK_PACE");
    if (!(o && o[0] == '0')) {
      ALLOC(x->pace, sizeof(unsigned long long) * wk::PACE_SLOTS);
      if (hipMemset(x->pace, 0, sizeof(unsigned long long) * wk::PACE_SLOTS) != hipSuccess) {
        x->err = "pacing table clear failed";
        return fail(WK_ERR_HIP);
      }
    }
  }
#undef ALLOC
  // synthetic randomisation of the initial state (BASELINE.json config 2 / 5)
  std::vector<float> dx(n, 0.0f);
  std::vector<int32_t> mt(n, WK_MAT_CARPET);
  for (size_t e = 0; e < n; e++) {
    uint32_t gid = (uint32_t)(c.EnvOffset + (int)e);
    if (c.RandomizeStart) dx[e] = wk::env_offset(seed, gid);
    if (c.RandomizeMaterial) mt[e] = wk::env_material(seed, gid);
  }
  if (hipMemcpy(x->dxoff, dx.data(), sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(x->mat, mt.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(x->rng_t, 0, sizeof(uint32_t) * n) != hipSuccess ||
      hipMemset(x->m, 0, sizeof(float) * np) != hipSuccess ||
      hipMemset(x->v, 0, sizeof(float) * np) != hipSuccess ||
      hipMemset(x->td, 0, n * T) != hipSuccess ||
      hipMemset(x->ep_acc, 0, sizeof(double) * n) != hipSuccess ||
      hipMemset(x->ep_len, 0, sizeof(int32_t) * n) != hipSuccess ||
      hipMemset(x->ep_rowcnt, 0, sizeof(uint32_t) * wk::episode_count_cells((int)n, T)) != hipSuccess ||
      hipMemset(x->ep_count, 0, sizeof(uint64_t)) != hipSuccess ||
      (x->gnorm && hipMemset(x->gnorm, 0, sizeof(wk::GradNormRec)) != hipSuccess)) {
    x->err = "initial upload failed";
    return fail(WK_ERR_HIP);
  }
  if (rough_order_upload(x, dx.data()) != hipSuccess) {
    x->err = "lane order upload failed";
    return fail(WK_ERR_HIP);
  }
  if (x->general) {
    const wk::NetDesc nets[2] = {x->net.critic, x->net.actor};
    if (hipMemcpy(x->net_dev, nets, sizeof nets, hipMemcpyHostToDevice) != hipSuccess) {
      x->err = "network description upload failed";
      return fail(WK_ERR_HIP);
    }
  }
  if (wk::launch_env_init(P, x->st, x->dxoff, nullptr, 0, x->stream) != hipSuccess ||
      wk::launch_xavier(x->W, seed, x->net.critic, x->net.actor, x->np, x->stream) != hipSuccess ||
      upload_image(x) != hipSuccess ||
      hipStreamSynchronize(x->stream) != hipSuccess) {
    x->err = "init kernels failed";
    return fail(WK_ERR_HIP);
  }
  *out = x;
  return WK_OK;
}

int wk_destroy(wk_ctx* c) {
  DevGuard dg_(c);
  if (!c) return WK_OK;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& e : c->pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  comm_close(c);
  for (void** p : c->owned)
    if (*p) (void)hipFree(*p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return WK_OK;
}

int wk_sync(wk_ctx* c) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  if (int r = rx_deferred(c)) return r;  // (an RCCL wk_rollout's record exchange: reported here)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_num_envs(const wk_ctx* c) { return c ? c->n : 0; }

int wk_reset(wk_ctx* c, const uint8_t* mask) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  const uint8_t* dmask = nullptr;
  if (mask) {
    if (ensure(c, &c->scratch, &c->scratch_bytes, c->n)) return WK_ERR_HIP;
    HIPCHK(c, hipMemcpyAsync(c->scratch, mask, c->n, hipMemcpyHostToDevice, c->stream));
    dmask = (const uint8_t*)c->scratch;
  }
  // Environment.Reset re-creates the walker after the floor (post-reset body order)
  HIPCHK(c, wk::launch_env_init(c->P, c->st, c->dxoff, dmask, 1, c->stream));
  HIPCHK(c, wk::launch_episode_reset(c->n, dmask, c->ep_acc, c->ep_len, c->stream));
  if (c->rn_acc) HIPCHK(c, wk::launch_rnorm_reset(c->n, dmask, c->rn_acc, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

int wk_set_materials(wk_ctx* c, const int32_t* mat_id) {
  DevGuard dg_(c);
  if (!c || !mat_id) return WK_ERR_ARG;
  for (int e = 0; e < c->n; e++)
    if (mat_id[e] < 0 || mat_id[e] > 7) { SETERR(c, "invalid material id %d at env %d", mat_id[e], e); return WK_ERR_ARG; }
  // the context's stream is non-blocking: queued rollouts read mat (also on auto-reset)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->mat, mat_id, sizeof(int32_t) * c->n, hipMemcpyHostToDevice));
  return WK_OK;
}

int wk_set_offsets(wk_ctx* c, const float* dx) {
  DevGuard dg_(c);
  if (!c || !dx) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // queued kernels read dxoff on auto-reset
  HIPCHK(c, hipMemcpy(c->dxoff, dx, sizeof(float) * c->n, hipMemcpyHostToDevice));
  HIPCHK(c, rough_order_upload(c, dx));
  return WK_OK;
}

int wk_get_weights(wk_ctx* c, float* p) {
  DevGuard dg_(c);
  if (!c || !p) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(p, c->W, sizeof(float) * c->np, hipMemcpyDeviceToHost));
  return WK_OK;
}
int wk_set_weights(wk_ctx* c, const float* p) {
  DevGuard dg_(c);
  if (!c || !p) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->W, p, sizeof(float) * c->np, hipMemcpyHostToDevice));
  HIPCHK(c, upload_image(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}
int wk_get_adam(wk_ctx* c, float* m, float* v, int* t) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (m) HIPCHK(c, hipMemcpy(m, c->m, sizeof(float) * c->np, hipMemcpyDeviceToHost));
  if (v) HIPCHK(c, hipMemcpy(v, c->v, sizeof(float) * c->np, hipMemcpyDeviceToHost));
  if (t) *t = c->adam_t;
  return WK_OK;
}
int wk_set_adam(wk_ctx* c, const float* m, const float* v, int t) {
  DevGuard dg_(c);
  if (!c || t < 0) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (m) HIPCHK(c, hipMemcpy(c->m, m, sizeof(float) * c->np, hipMemcpyHostToDevice));
  if (v) HIPCHK(c, hipMemcpy(c->v, v, sizeof(float) * c->np, hipMemcpyHostToDevice));
  c->adam_t = t;
  return WK_OK;
}

int wk_set_learning_rate(wk_ctx* c, float alpha) {
  if (!c || !std::isfinite(alpha) || alpha < 0.0f) return WK_ERR_ARG;
  c->cfg.Alpha = alpha;  // adam_args reads it at every step, on every path
  return WK_OK;
}

int wk_get_learning_rate(wk_ctx* c, float* alpha) {
  if (!c || !alpha) return WK_ERR_ARG;
  *alpha = c->cfg.Alpha;
  return WK_OK;
}

int wk_profile_enable(wk_ctx* c, int on) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  c->prof = on < 0 ? 0 : (on > 2 ? 2 : on);
  return WK_OK;
}

int wk_profile_reset(wk_ctx* c) {
  DevGuard dg_(c);
  if (!c) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  for (int i = 0; i < PK_N; i++) { c->prof_ms[i] = 0; c->prof_cnt[i] = 0; }
  c->prof_units = 0;
  return WK_OK;
}

int wk_profile_get(wk_ctx* c, wk_profile* o) {
  DevGuard dg_(c);
  if (!c || !o) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  o->physics_ms = c->prof_ms[PK_PHYS]; o->physics_launches = c->prof_cnt[PK_PHYS];
  o->physics_env_steps = c->prof_units;
  o->grad_ms = c->prof_ms[PK_GRAD]; o->grad_launches = c->prof_cnt[PK_GRAD];
  o->reduce_ms = c->prof_ms[PK_REDUCE]; o->reduce_launches = c->prof_cnt[PK_REDUCE];
  o->adam_ms = c->prof_ms[PK_ADAM]; o->adam_launches = c->prof_cnt[PK_ADAM];
  o->allreduce_ms = c->prof_ms[PK_ALLRED]; o->allreduce_calls = c->prof_cnt[PK_ALLRED];
  o->returns_ms = c->prof_ms[PK_RET]; o->returns_launches = c->prof_cnt[PK_RET];
  o->update_ms = c->prof_ms[PK_UPDATE]; o->update_calls = c->prof_cnt[PK_UPDATE];
  return WK_OK;
}
