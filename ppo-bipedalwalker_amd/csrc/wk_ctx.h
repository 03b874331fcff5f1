// wk_ctx.h -- the context behind the C ABI (include/wk_api.h) and what the host units
// (wk_api*.cpp) share: the entry points' guards, the allocator and carver, and the helpers a second
// unit calls.  Private: not installed, and hidden from the library's dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/wk_api.h"
#include "wk_common.h"
#include "wk_kernels.h"
#include "wk_net.h"

struct ncclComm;  // RCCL's opaque communicator: its header is wk_api_comm.cpp's alone
typedef struct ncclComm* ncclComm_t;

#pragma GCC visibility push(hidden)

// level 1: one event pair per rollout / returns / whole PPO update (cheap enough for a
// timed loop); level 2 adds one per gradient / reduce / all-reduce / Adam launch
enum ProfKind { PK_PHYS = 0, PK_GRAD, PK_REDUCE, PK_ADAM, PK_ALLRED, PK_RET, PK_UPDATE, PK_N };

struct wk_ctx {
  wk_config cfg;
  int grad_impl = -1;  // matrix-core gradient kernel (wk::GI_*; -1 = by minibatch size)
  // the networks: NetworkKernels = 0 runs the built-in kernels on the default strings, 1 the
  // general kernels (wk_net.hip) on `net`; np / slabn size every parameter-shaped buffer
  bool general = false;
  wk::NetSpec net;
  wk::NetDesc* net_dev = nullptr;  // device copy {critic, actor}
  int act_rows = 0;
  int np = wk::NPARAM, slabn = wk::SLAB;
  int device = 0;
  int n = 0;
  uint64_t seed = 0;
  hipStream_t stream = nullptr;
  std::string err;
  wk::EnvParams P{};
  float lp_const = 0.0f;
  // env
  float* st = nullptr;        // walker records [n][NSTATE]
  float* dxoff = nullptr;     // [n]
  int32_t* mat = nullptr;     // [n]
  uint32_t* rng_t = nullptr;  // [n]
  // params
  float* W = nullptr; float* m = nullptr; float* v = nullptr; float* grad = nullptr;
  float* Wz = nullptr;        // W in the matrix-core operand order (wk_mfma_layout.h)
  int adam_t = 0;
  // trajectory [T][n]
  int T = 0, T_valid = 0;
  float *ts = nullptr, *ta = nullptr, *tlp = nullptr, *tr = nullptr, *tv = nullptr, *tret = nullptr, *tadv = nullptr;
  uint8_t* td = nullptr;
  bool returns_valid = false;
  // ReturnsMode = 1: the value each walker's reverse scan starts from (part of the trajectory)
  float* vlast = nullptr;     // [n]
  bool vlast_valid = false;
  // TargetKL > 0: the last per-epoch check of the last wk_ppo_update (wk_update_stats_get)
  wk_ppo_stats upd_stats{};
  bool upd_stats_valid = false;
  // MaxGradNorm > 0: the device record of the Adam steps' gradient norms (wk_grad_norms_get) and
  // the steps launched since it was last cleared
  wk::GradNormRec* gnorm = nullptr;
  int64_t gnorm_steps = 0;
  // LearnLogStd = 1: the host's Adam step on the scalar log-std (P.log_std holds the value itself
  // on every context) and the counters of the last wk_ppo_update (wk_get_log_std)
  struct LogStd {
    double m = 0.0, v = 0.0, grad_last = 0.0;
    int t = 0;
    int64_t steps = 0, clamped = 0, nonfinite = 0;
  } ls;
  // reward normalisation (wk_reward_norm_config): nothing is allocated before the first enable.
  // rn_acc [n] the walkers' running discounted returns, rn_rec the statistics and the scale, trs
  // [T][n] the scaled rewards the returns kernels read, rn_partial the scan's tile partials,
  // rn_snap wk_snapshot's copy of rn_acc and rn_rec
  bool rn_ever = false;
  int rn_on = 0, rn_frozen = 0;
  float rn_clip = 10.0f, rn_eps = 1e-8f;
  float* rn_acc = nullptr; float* trs = nullptr;
  wk::RnormRec* rn_rec = nullptr;
  unsigned long long* rn_partial = nullptr;
  char* rn_snap = nullptr;
  bool rn_snap_valid = false;
  // data collection (ConsoleRenderer.AddTotalEpisodeReward / AddCriticLoss / AddActorLoss)
  int collect = 1;
  uint32_t rollout_steps = 0;  // env-steps taken by wk_rollout so far (episode log clock)
  double* ep_acc = nullptr;       // [n] running episode reward
  int32_t* ep_len = nullptr;      // [n]
  void* ep_scratch = nullptr;     // [T][n] float2
  uint32_t* ep_rowcnt = nullptr;  // [T][tiles] episode counts per (row, 4,096-walker tile)
  uint64_t* ep_count = nullptr;   // device: records appended since the last drain
  wk::EpisodeRecDev* ep_log = nullptr;
  uint64_t ep_cap = 0;
  float* loss_log = nullptr;      // [loss_cap][2] (critic, actor) per PPO update
  uint64_t loss_count = 0, loss_cap = 0;
  // dev_alloc's record: the addresses of the pointers whose buffers wk_destroy frees (the IPC
  // region xch and its peers have their own calls); props takes its block over from props_next
  std::vector<void**> owned{(void**)&props};
  // scratch.  Two buffers for temporaries, because net_sampled (scratch) runs inside callers that
  // hold pointers into their own carve-up (wk_step_sampled: scratch2), and growing one frees it
  float* partial = nullptr; size_t partial_bytes = 0;
  void* scratch = nullptr; size_t scratch_bytes = 0;  // net_sampled, wk_get_obs, wk_reset, bootstrap_values, wk_allreduce_test
  void* scratch2 = nullptr; size_t scratch2_bytes = 0;  // the entry points that carve
  // wk_evaluate's private block (allocated on first use, carved per call): walker records, Philox
  // counters, props, lane order, running episodes, records, the physics row and the fold's records
  void* ev = nullptr; size_t ev_bytes = 0;
  struct EvalBlock {
    float* st; uint32_t* rng_t; float* props; int32_t* order; uint32_t* order_cnt;
    float *obs, *act, *rew, *pos; uint8_t* done; uint32_t* fault;
    unsigned long long *partial, *out;
    wk::EvalArgs a;  // the running episodes, the records, the running count
    bool valid = false;
  } evb{};
  // the frame renderer's buffers (wk_render*; grown on demand, kept between calls): the views'
  // walker ids, wk_render_states' records and the host variants' device image
  int32_t* rd_envs = nullptr; size_t rd_envs_bytes = 0;
  float* rd_states = nullptr; size_t rd_states_bytes = 0;
  uint32_t* rd_img = nullptr; size_t rd_img_bytes = 0;
  // scene props (wk_set_scene): descriptions, kernel constants, [n][pstride] state
  std::vector<wk_prop> scene_desc;
  wk::SceneDev scene{};
  float* props = nullptr;
  float* props_next = nullptr;  // wk_set_scene's new block until it replaces props
  // wk_snapshot: one device block holding every snapshotted buffer, plus the host scalars
  void* snap = nullptr; size_t snap_bytes = 0;
  struct SnapHost {
    int adam_t = 0;
    float log_std = 0.0f; LogStd ls;  // LearnLogStd = 1 (with what wk_get_log_std reports)
    uint32_t rollout_steps = 0;
    uint64_t loss_count = 0;
  } snap_host;
  bool snap_valid = false;
  bool snap_log_drained = false;  // wk_episode_log_drain since the save: the saved count's records are gone
  unsigned long long* counts = nullptr;  // [WK_NEV] device (wk_count_events)
  int32_t* order = nullptr;       // [n] lane order of the split physics kernels (null: identity)
  uint32_t* order_cnt = nullptr;  // [order_cells(n)] episode-0 walkers per tile + swap count
  unsigned long long* pace = nullptr;  // [PACE_SLOTS] per-SIMD progress tags of the env-step kernels
  uint32_t pace_seq = 0;
  // comm
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1;
  wk_host_allreduce_fn host_ar = nullptr;  // wk_comm_init_host: a caller-supplied all-reduce
  void* host_ar_user = nullptr;
  std::vector<float> host_ar_buf;
  // wk_comm_records: the exchange of statistics records (RX_*: declared kind; it runs once the
  // matching communicator exists).  rx_dev [nranks][RECORD_WORDS] is the device gather buffer, this
  // rank's record in slot `rank`; rx_err the device word k_rnorm_merge leaves a header mismatch in,
  // read by the next synchronising call while rx_pending (an RCCL wk_rollout does not wait)
  enum { RX_NONE = 0, RX_RCCL = 1, RX_HOST = 2 };
  int rx_kind = RX_NONE;
  wk_host_allgather_fn* rx_fn = nullptr;
  void* rx_user = nullptr;
  uint64_t rx_seq = 0;                 // record exchanges so far (the header's sequence)
  unsigned long long* rx_dev = nullptr;
  uint32_t* rx_err = nullptr;
  bool rx_pending = false;
  std::vector<uint64_t> rx_host;       // [nranks][RECORD_WORDS] on the host
  // wk_comm_init_ipc: the one-shot exchange over peer-mapped memory (k_reduce_xch_adam)
  void* xch = nullptr;                 // this rank's exchange region (exported by IPC handle)
  std::vector<void*> xch_peers;        // peers' regions, opened from their handles
  wk::XchArgs xa{};                    // slab / flag pointers of every rank
  bool ipc = false;
  uint64_t xch_seq = 0;
  uint32_t* xch_err = nullptr;         // device word: a peer never published
  bool xch_uncached = false;           // the region is uncached device memory (else hipMalloc)
  uint64_t xch_timeout_ticks = 0;      // bounded peer wait (WK_XCH_TIMEOUT_S / wk_comm_set_timeout)
  uint64_t* xch_stamps = nullptr;      // wk_comm_xch_profile: [cap][blocks][XCH_POINTS] clock ring
  int xch_stamp_cap = 0;
  int64_t xch_stamp_launches = 0;      // launches stamped since the ring was (re)armed
  // the reference's per-body call shape (wk_take_actions / wk_object_update)
  std::vector<float> pend;             // [n][4] torques wk_take_actions stored for the next frame
  std::vector<uint8_t> pend_set;       // [n] walker given torques since the last frame
  int64_t frame_calls = 0, frame_len = 0;
  // profiling
  int prof = 0;  // profile level
  struct Ev { int kind; hipEvent_t a, b; int64_t units; };
  std::vector<Ev> pending;
  std::vector<hipEvent_t> pool;
  double prof_ms[PK_N] = {0};
  int64_t prof_cnt[PK_N] = {0};
  int64_t prof_units = 0;
};

// Every entry point binds the context's device for its duration: buffers are
// allocated and copied on c->device whatever the calling thread's current device is, and the
// caller's current device is restored afterwards.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(const wk_ctx* c) {
    if (c && hipGetDevice(&prev) == hipSuccess && prev != c->device)
      switched = hipSetDevice(c->device) == hipSuccess;
  }
  ~DevGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

#define SETERR(ctx, ...)                                           \
  do {                                                             \
    char _b[512];                                                  \
    snprintf(_b, sizeof(_b), __VA_ARGS__);                         \
    (ctx)->err = _b;                                               \
  } while (0)

#define HIPCHK(ctx, call)                                                               \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess) {                                                             \
      SETERR(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      return WK_ERR_HIP;                                                                \
    }                                                                                   \
  } while (0)

hipEvent_t ev_get(wk_ctx* c);  // an event from the context's pool (wk_api.cpp)

struct ProfScope {
  wk_ctx* c; int kind; int64_t units; hipEvent_t a = nullptr, b = nullptr;
  bool on;
  ProfScope(wk_ctx* c_, int k, int64_t u = 0, int level = 1)
      : c(c_), kind(k), units(u), on(c_->prof >= level) {
    if (on) {
      a = ev_get(c); b = ev_get(c);
      if (a) (void)hipEventRecord(a, c->stream);
    }
  }
  ~ProfScope() {
    if (on && a && b) {
      (void)hipEventRecord(b, c->stream);
      c->pending.push_back({kind, a, b, units});
    }
  }
};

// The one allocator: hipMalloc through `p`, recording p's address (once).  wk_destroy frees what
// the recorded pointers hold by then, so a buffer replaced through its pointer is freed once.
template <class T>
hipError_t dev_alloc(wk_ctx* c, T** p, size_t bytes) {
  const hipError_t e = hipMalloc((void**)p, bytes);
  if (e == hipSuccess && std::find(c->owned.begin(), c->owned.end(), (void**)p) == c->owned.end())
    c->owned.push_back((void**)p);
  return e;
}

// a lazily sized buffer: at least `need` bytes behind *p (the contents are not kept)
template <class T>
int ensure(wk_ctx* c, T** p, size_t* have, size_t need) {
  if (*have >= need) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  HIPCHK(c, dev_alloc(c, p, need));
  *have = need;
  return 0;
}

// The bump carver over a scratch buffer: the caller lists its pieces once (where the pointer goes,
// how many bytes); each is aligned to 256 bytes, and a piece of no bytes gets null.
struct Piece { void* out; size_t bytes; };  // out: the address of the pointer
inline int carve(wk_ctx* c, void** buf, size_t* have, std::initializer_list<Piece> pieces) {
  const auto span = [](const Piece& p) { return (p.bytes + 255) & ~(size_t)255; };
  size_t total = 0;
  for (const Piece& p : pieces) total += span(p);
  if (ensure(c, buf, have, total)) return WK_ERR_HIP;
  char* at = (char*)*buf;
  for (const Piece& p : pieces) {
    *(void**)p.out = p.bytes ? at : nullptr;
    at += span(p);
  }
  return WK_OK;
}

// a device buffer and its size: the rows of wk_snapshot's block and of the checkpoint file
struct Seg { void* p; size_t bytes; };

// one of the eight [T][n] trajectory rows, with bytes per sample
struct TrajRow { const char* name; void** p; size_t bytes; };

// The helpers a second unit calls, under the unit that defines them.
// wk_api.cpp
std::array<TrajRow, 8> traj_rows(wk_ctx* c);
hipError_t rough_order_upload(wk_ctx* c, const float* dx_host);
hipError_t upload_image(wk_ctx* c);
void apply_log_std(wk_ctx* c, float log_std);
// wk_api_env.cpp
hipError_t launch_physics(wk_ctx* c, int mode, wk::StepArgs& A, float* props, int32_t* order,
                          uint32_t* order_cnt);
wk::StepArgs policy_args(wk_ctx* c);
hipError_t launch_policy_for(wk_ctx* c, int n, const float* obs, const int32_t* ids,
                             const uint32_t* steps, float* mean, float* act, float* logp, float* v);
int sampled_steps(wk_ctx* c, wk::StepArgs& A);
int check_state_or_fail(wk_ctx* c, const float* state);
int prop_vertices(const wk_prop& p, int smooth, float* xs, float* ys);
// wk_api_rollout.cpp
int returns_impl(wk_ctx* c);
// wk_api_comm.cpp
uint64_t* xch_stamp_slot(wk_ctx* c);
int comm_exchange(wk_ctx* c);
int xch_status(wk_ctx* c);
int xch_mark_t(wk_ctx* c);
void comm_close(wk_ctx* c);
// the record exchange (wk_comm_records).  records_on: declared and the communicator exists.
// rx_header: the next exchange's header word (advances the sequence).  rx_gather_device: this
// rank's record in its slot of rx_dev -> every rank's in rx_dev (RCCL: stream-ordered, no wait, the
// header check left to the consumer kernel and rx_deferred; host: checked here).  rx_gather_host:
// the same, then every rank's record on the host in c->rx_host, headers checked (it synchronises).
// rx_deferred: the pending header check of an RCCL reward-normalisation exchange (it synchronises).
inline bool records_on(const wk_ctx* c) {
  return c->rx_kind != wk_ctx::RX_NONE && (c->comm != nullptr || c->host_ar != nullptr);
}
uint64_t rx_header(wk_ctx* c, int kind);
int rx_gather_device(wk_ctx* c, uint64_t header);
int rx_gather_host(wk_ctx* c, uint64_t header);
int rx_deferred(wk_ctx* c);
// wk_api_io.cpp
bool write_file(const char* path, const void* data, size_t n);

#pragma GCC visibility pop
