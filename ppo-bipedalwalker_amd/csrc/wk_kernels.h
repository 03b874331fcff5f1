// wk_kernels.h -- kernel argument blocks and host launch shims: what every kernel unit (*.hip)
// offers the host units (wk_api*.cpp) and the other kernel units.  One heading per unit, in the
// Makefile's order; an argument block several units share comes before the first that takes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wk_common.h"
#include "wk_net.h"

namespace wk {

// ---- the rollout units: wk_env_*.hip, wk_env.hip
// per-substep pair bookkeeping; layout == wk_pair_trace (include/wk_api.h)
struct PairTraceDev {
  uint8_t aabb_hit[9];
  uint8_t sat_hit[9];
  uint8_t n_contacts[9];
  uint8_t pad[5];
  float normal[9][2];
  float depth[9];
  float contact[9][2][2];
  float impulse[9][2];
  float joint_depth[4];
  float joint_impulse[4];
};

// physics event counters of the counting replay (wk_count_events; SURVEY 8(d) F_counted)
enum : int {
  EV_JOINT = 0,                            // Joint.Step past the 0.1 gap early-out
  EV_AABB_LL, EV_AABB_LF, EV_AABB_BF,      // bounding boxes overlap -> SAT runs
  EV_SAT_LL, EV_SAT_LF, EV_SAT_BF,         // SAT reports a collision -> contacts + MoveObjects
  EV_IMP_LL, EV_IMP_LF, EV_IMP_BF,         // >= 1 contact point -> the impulse pair
  EV_CONTACTS,                             // contact points found
  EV_SUBSTEPS,                             // walker-substeps
  EV_ENV_STEPS, EV_RESETS,                 // env-steps, auto-resets
  EV_STEPS_LF, EV_STEPS_SATLL,             // walker env-steps with >= 1 leg-floor AABB hit /
                                           // >= 1 leg-leg SAT hit (how concentrated they are)
  NEV = 16                                 // (LL leg-leg, LF leg-floor, BF torso-floor)
};

struct StepArgs {
  float* st;                 // walker state records [n][NSTATE]
  const float* dxoff;        // [n] start offset (x = 125 + dx)
  const int32_t* mat;        // [n] material id
  uint32_t* rng_t;           // [n] per-env env-step counter (Philox counter)
  const float* actions;      // [k][n][4] or null (policy)
  float* obs_out;            // [k][n][12] or null
  float* pos_out;            // [k][n][2] torso centroid after the step, before any auto-reset
                             // (Walker.GetPosition at Environment.cs:119) or null
  float* rew_out;            // [k][n] or null
  uint8_t* done_out;         // [k][n] or null
  uint32_t* fault_out;       // [n] or null (OR-accumulated)
  const float* W;            // params (policy)
  const float* Wz;           // params in the matrix-core operand order (wk_mfma_layout.h)
  float lp_const;            // -ln(std) - ln(sqrt(2 pi))
  // trajectory buffer (RECORD), index t*n + e
  float* traj_s; float* traj_a; float* traj_lp; float* traj_r; uint8_t* traj_d; float* traj_v;
  int t0;
  PairTraceDev* trace;       // [n][iterations] (TRACE)
  int k_steps;
  float* props;              // scene props [n][SceneDev::pstride] (k_env_scene) or null
  unsigned long long* counts;  // [NEV] event totals (counting replay, mode 4) or null
  const int32_t* order;      // k_env_side: walker of lane slot s (wk_order.hip) or null (identity)
  // k_env_side pair mapping / k_env_step: per-SIMD progress tags of the co-resident waves
  // ([PACE_SLOTS], zeroed at creation; null: no pacing) and this launch's sequence number
  unsigned long long* pace;
  uint32_t pace_seq;
};
enum : int { PACE_SLOTS = 8 * 8 * 2 * 16 * 4 };  // XCC x SE x SH x CU x SIMD (HW_ID fields)
// threads per block of the split (pair / quad) rollout kernels; wk_rollout_mapping reports the
// launched grid from it
#ifndef WK_SIDE_BLOCK
#define WK_SIDE_BLOCK 256
#endif
constexpr int SIDE_BLOCK_THREADS = WK_SIDE_BLOCK;

// scene props (wk_env_scene.h): Square / Triangle / Hexagon bodies after the floor, the same
// shapes for every walker; per walker and prop k the state x[nv], y[nv], cx, cy, vx, vy, w,
// angle starts at float off[k] of the walker's prop record
enum : int {
  SCENE_MAX_PROPS = 4, SCENE_PROP_MAXV = 24, SCENE_MAX_VERTS = 32,
  SCENE_FIELDS = 2 * SCENE_MAX_VERTS + 6 * SCENE_MAX_PROPS
};
struct SceneDev {
  int n_props, pstride;
  int nv[SCENE_MAX_PROPS], off[SCENE_MAX_PROPS], stat[SCENE_MAX_PROPS];
  float im[SCENE_MAX_PROPS], ii[SCENE_MAX_PROPS], e[SCENE_MAX_PROPS], mu[SCENE_MAX_PROPS];
  float adx[SCENE_MAX_PROPS], ady[SCENE_MAX_PROPS];  // acceleration * deltaTime
};

hipError_t launch_env_step(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s);
hipError_t launch_env_scene(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                            hipStream_t s);
// what the two dispatchers above (wk_env.hip) choose between: one kernel family per translation
// unit, wk_env_pair.hip, wk_env_quad.hip, wk_env_side_rough.hip (k_env_side) and
// wk_env_scene_{given,policy}[_rough].hip (k_env_scene), each built with its own switches and flags
void launch_side_pair(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s);
void launch_side_quad(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s);
void launch_side_pair_rough(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s);
void launch_side_quad_rough(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s);
void launch_env_scene_given(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                            hipStream_t s);
void launch_env_scene_policy(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                             hipStream_t s);
void launch_env_scene_given_rough(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                                  hipStream_t s);
void launch_env_scene_policy_rough(int mode, const EnvParams& P, const StepArgs& A, const SceneDev& S,
                                   hipStream_t s);
hipError_t launch_env_init(const EnvParams& P, float* st, const float* dx, const uint8_t* mask,
                           int post, hipStream_t s);
hipError_t launch_get_obs(const EnvParams& P, const float* st, float* obs, hipStream_t s);
hipError_t launch_policy(const EnvParams& P, const float* W, float lp_const, int n,
                         const float* obs, const int32_t* env_ids, const uint32_t* steps,
                         float* mean, float* act, float* logp, float* v, hipStream_t s);

// ---- the update path's argument blocks (wk_ppo*.hip, wk_tail.hip, wk_stats.hip, wk_net.hip)
struct AdamArgs {
  float* W; float* m; float* v; const float* grad;
  float* Wz;  // operand-order image kept in step with W (or null)
  float c1, c2, beta1, beta2, bc1, bc2, alpha, eps;
};

struct GradArgs {
  const float* W;        // params
  const float* Wz;       // the same params in the matrix-core operand order (wk_mfma_layout.h)
  const float* states;   // [P][12]
  const float* actions;  // [P][4]
  const float* logp_old; // [P][4]
  const float* returns;  // [P]
  const float* adv;      // [P]
  uint32_t pool;         // P
  uint32_t base;         // first permuted position of this minibatch
  int use_perm;
  PermKey pk;
  int samples;           // samples in this minibatch (local)
  int spw;               // the sequential kernel's samples per wave (launch_ppo_grad sets it to
                         // samples; no one else reads it).  It stays: without it every later
                         // argument moves, and the compiler then regroups the scalar loads and
                         // reschedules every gradient kernel instead of only changing offsets
                         // (profiles/prune_update_path.txt)
  float b_div;           // divisor of dV / dmu (BatchSize / global minibatch)
  float std_;            // MathF.Exp(LogStandardDeviation)
  float lp_const;        // -ln(std) - ln(sqrt(2 pi))
  float upper, lower;    // 1 + eps, 1 - eps
  float* partial;        // [nblocks][SLAB]
};

// gradient + critic diag, actor diag, skipped, then zero pads to a multiple of 4 floats (16-byte
// rows: the matrix-core kernel's block fold and slab stores are f4-wide)
enum : int { SLAB = (NPARAM + 3 + 3) / 4 * 4 };
static_assert(SLAB % 4 == 0 && SLAB >= NPARAM + 3, "slab layout");
// the ordered reduction of a gradient launch's block slabs (wk_tail.h): groups of RG consecutive
// slabs in order, then up to RG groups in order -- no gradient launch writes more slabs
enum { RG = 16 };
enum : int { GRAD_MAX_BLOCKS = RG * RG };

// ---- wk_ppo.hip
// the sequential lane-per-neuron kernel: one slab
hipError_t launch_ppo_grad(GradArgs g, hipStream_t s);
hipError_t configure_device_kernels();  // dynamic-LDS attributes, current device (wk_create)

// ---- wk_ppo_mfma.hip
hipError_t configure_mfma_kernels();
// matrix-core gradient kernels: producer / consumer pairs (ws), tile-parallel teams of four
// waves, two (tp) or one (tp1) per block, one wave per chunk (mf); GI_AUTO picks by size
enum : int { GI_AUTO = -1, GI_WS = 0, GI_TP2 = 1, GI_TP1 = 2, GI_MF = 3 };
int grad_impl_env();                       // WK_GRAD_IMPL = ws / tp / tp1 / mf, else GI_AUTO
int grad_impl_for(int impl, int samples);  // resolves GI_AUTO
hipError_t launch_ppo_grad_mfma(const GradArgs& g, int nblocks, int impl, hipStream_t s);
hipError_t launch_swizzle(const float* W, float* Wz, hipStream_t s);
int mfma_image_floats();
int ppo_grad_mfma_blocks(int samples, int impl);

// ---- wk_tail.hip: block slabs -> weight step
// nblocks <= GRAD_MAX_BLOCKS slabs -> grad [SLAB]; adam: applied in the same launch, or null
hipError_t launch_grad_reduce(const float* partial, int nblocks, float* grad, const AdamArgs* adam,
                              hipStream_t s);
// the general networks' slabs (net_slab_floats(np) floats each); a.W set: Adam as well
hipError_t launch_net_reduce(const float* partial, int nblocks, int np, float* grad, const AdamArgs& a,
                             hipStream_t s);
hipError_t launch_adam(const AdamArgs& a, hipStream_t s);
// MaxGradNorm > 0 (k_clip_adam): per-network gradient-norm clipping and Adam over
// a.grad[0..np) of either kernel family, critic [0, n_critic) and actor [n_critic, np), and the
// device record of the norms; layout == wk_grad_norms (include/wk_api.h)
struct GradNormRec {
  long long steps;
  long long clipped[2];
  long long nonfinite[2];
  double norm_last[2], norm_max[2], norm_sum[2];
  float scale_last[2];
  int32_t pad[2];
};
static_assert(sizeof(GradNormRec) == 104, "GradNormRec is wk_grad_norms");
hipError_t launch_clip_adam(const AdamArgs& a, int np, int n_critic, float max_norm, GradNormRec* rec,
                            hipStream_t s);

// One-shot gradient exchange over peer-mapped (IPC) memory, fused with the ordered block
// reduction and Adam (wk_comm_init_ipc): rank r's exchange region is [2][SLAB] floats
// (double-buffered by minibatch parity) then XCH_FLAGS uint64 sequence flags, one per block of
// the fused kernel (each block owns a span of parameter quads).
// XCH_TIMEOUT_S_DEFAULT: the bounded wait for a peer's flag (s_memrealtime ticks of the 100 MHz
// constant clock, XCH_TICKS_PER_S); a context takes WK_XCH_TIMEOUT_S from the environment at
// wk_comm_init_ipc or wk_comm_set_timeout.  XCH_ABORT: the flag value of a rank whose exchange
// timed out (or that saw an earlier timeout): a peer that reads it fails the same minibatch
// instead of applying it.  XCH_MAX_RANKS_PER_DEVICE: more ranks sharing one GPU stall (their
// waiting exchange blocks hold the CUs a peer's gradient kernel needs), so wk_comm_init_ipc
// refuses them.
enum : int { XCH_FLAGS = 128, XCH_MAX_RANKS = 8, XCH_MAX_RANKS_PER_DEVICE = 4 };
constexpr double XCH_TIMEOUT_S_DEFAULT = 30.0;
constexpr double XCH_TICKS_PER_S = 1.0e8;
constexpr uint64_t XCH_ABORT = ~0ull;
struct XchArgs {
  const float* partial;                // this rank's gradient-kernel block slabs [nblocks][SLAB]
  int nblocks;
  float* grad_out;                     // the rank-order sum over ranks [SLAB]
  float* slab[XCH_MAX_RANKS];          // every rank's exchange region (own + peer-mapped)
  uint64_t* flag[XCH_MAX_RANKS];       // every rank's XCH_BLOCKS flags
  int rank, nranks;
  uint64_t seq;                        // this minibatch's sequence number (from 1)
  uint32_t* err;                       // [0] set to 1 if a peer never published (bounded wait) or
                                       // aborted; once set, every later exchange is a no-op (no
                                       // Adam); [1] the Adam step t block 0 last applied
  uint64_t timeout_ticks;              // the bounded wait (s_memrealtime ticks)
  uint32_t t;                          // this minibatch's Adam step (with a.W)
  AdamArgs a;                          // a.W == null: exchange only (gradient-only calls)
  uint64_t* stamps;                    // null, or this launch's [blocks][XCH_POINTS] clock stamps
};
// exchange timing (wk_comm_xch_profile): per block, the 100 MHz constant clock at entry, slab
// published, every peer's flag seen, exit
enum : int { XCH_POINTS = 4 };
int xch_blocks();
size_t xch_region_bytes();
hipError_t launch_reduce_xch_adam(const XchArgs& x, hipStream_t s);

// ---- wk_returns.hip: returns and advantages over the [T][n] rows.  mode: ReturnsMode -- 0 the
// reference's scan (k_returns), 1 chained GAE(lambda) and the scan bootstrapped from vlast[n]
// (k_returns_std), the only mode that reads vlast
hipError_t launch_returns(int mode, int n, int T, int use_gae, float gamma, float lambda, const float* r,
                          const float* v, const uint8_t* d, const float* vlast, float* ret, float* adv,
                          hipStream_t s);
hipError_t launch_normalize(float* x, int n, float eps, hipStream_t s);

// ---- wk_stats.hip
// Policy statistics over the trajectory (wk_policy_stats; k_ppo_stats in wk_stats.hip for the
// built-in networks, k_net_stats in wk_net.hip for the general ones, wk_stats.h the arithmetic
// they share).  StatsRec is the record every stage carries -- counts as integers, sums in double,
// the largest ratio -- as STATS_FIELDS 64-bit words: one per block from the forward kernel, one
// from k_stats_finish (the blocks' records in block order), which the host divides.
struct StatsRec {
  long long rows, skipped, clipped;  // counted rows, skipped rows, clipped (row, dim) entries
  double kl, k1, surr;               // over counted entries: expm1(d) - d, -d, min(r adv, clip(r) adv)
  double sr, srr, se, see;           // over counted rows: ret, ret^2, e = ret - V, e^2
  double rmax;                       // largest ratio (-inf: none; a NaN stays)
};
enum : int { STATS_FIELDS = 11, STATS_COUNTS = 3, STATS_RMAX = 10 };
static_assert(sizeof(StatsRec) == 8 * STATS_FIELDS, "StatsRec is STATS_FIELDS 64-bit words");
// The log-std pass (wk_log_std_gradient, a LearnLogStd = 1 update): the <true> instantiation of
// the same passes (kernels k_ppo_logstd and k_net_logstd) carries two trailing sums in double over
// the counted entries -- the clipped surrogate's derivative by lp times d lp / d log_std = zz - 1,
// and zz = ((act - mean) / std)^2.  StatsRec and STATS_FIELDS are the <false> instantiation's
// (k_ppo_stats, k_net_stats), as before.
struct StatsRecLS {
  StatsRec s;
  double term, zz;
};
enum : int { STATS_FIELDS_LS = STATS_FIELDS + 2 };
static_assert(sizeof(StatsRecLS) == 8 * STATS_FIELDS_LS, "StatsRecLS is STATS_FIELDS_LS 64-bit words");
// the built-in kernel's grid: at most STATS_MAX_BLOCKS blocks of STATS_WAVES waves, every wave
// striding over the 16-row chunks (one grid pass = STATS_MAX_BLOCKS * STATS_WAVES * 16 rows)
enum : int { STATS_MAX_BLOCKS = 512, STATS_WAVES = 4 };
struct StatsArgs {
  GradArgs g;               // the rows in buffer order: samples = rows, base 0, no permutation
  float* logp_new;          // [rows][4] or null
  float* values_new;        // [rows] or null
  unsigned long long* partial;  // [blocks][STATS_FIELDS], log_std: [blocks][STATS_FIELDS_LS]
};
// log_std: the <true> instantiation and its record width, in all three launches (with wk_net.hip's)
int ppo_stats_blocks(int rows);
hipError_t launch_ppo_stats(const StatsArgs& a, int nblocks, bool log_std, hipStream_t s);
hipError_t launch_stats_finish(const unsigned long long* partial, int nblocks, bool log_std, void* out,
                               hipStream_t s);

// ---- wk_rnorm.hip
// Reward normalisation (wk_reward_norm_*; wk_rnorm.hip): rewards scaled by the running standard
// deviation of the walkers' discounted returns, into a second reward buffer that only the returns
// kernels read.  RnormRec is the device record; layout == wk_reward_norm (include/wk_api.h), the
// configuration fields (clip, epsilon, enabled, frozen) filled by the host when it is read.
struct RnormRec {
  long long count;
  double mean, m2, var;
  float scale, clip, epsilon;
  int32_t enabled, frozen, pad;
  long long rows, clipped, nonfinite;
};
static_assert(sizeof(RnormRec) == 80, "RnormRec is wk_reward_norm");
// the scan's tile: RNORM_TILE walkers, one lane each, fold to one partial of RNORM_FIELDS 64-bit
// words (samples, non-finite samples as integers; sum x, sum x^2 as doubles).  The association is
// a function of n alone: a tree over the tile's lanes, then the tiles in tile order.
enum : int { RNORM_TILE = 256, RNORM_FIELDS = 4 };
int rnorm_tiles(int n);
// the full pass: scan (acc carried, partial[rnorm_tiles(n)][RNORM_FIELDS]), finish (the merge into
// rec and the new scale), apply (out = clamp(r * rec->scale)).  learn = false: finish only clears
// the last pass's counters and the scan does not run -- the apply step with the scale as it is.
hipError_t launch_rnorm_pass(int n, int T, float gamma, float clip, float epsilon, bool learn,
                             const float* r, const uint8_t* done, float* acc,
                             unsigned long long* partial, RnormRec* rec, float* out, hipStream_t s);
hipError_t launch_rnorm_reset(int n, const uint8_t* mask, float* acc, hipStream_t s);
// The full pass on a record-exchange context (wk_comm_records), in two halves around the gather.
// A record is RECORD_WORDS 64-bit words, word 0 its header; `slot` is this rank's record in the
// device gather buffer all[nranks][RECORD_WORDS].
//   launch_rnorm_batch  scan, then k_rnorm_batch: the tiles' partials folded with k_rnorm_finish's
//                       association into (count, bad, sum x, sum x^2) behind the header in slot
//   launch_rnorm_merge  k_rnorm_merge: the ranks' records folded in rank order from rank 0's and
//                       merged into rec with k_rnorm_finish's arithmetic (a record whose header is
//                       not `header` puts its rank + 1 in *err and nothing is merged), then apply
enum : int { RECORD_WORDS = 16 };
hipError_t launch_rnorm_batch(int n, int T, float gamma, const float* r, const uint8_t* done, float* acc,
                              unsigned long long* partial, unsigned long long header,
                              unsigned long long* slot, hipStream_t s);
hipError_t launch_rnorm_merge(int n, int T, float clip, float epsilon, const unsigned long long* all,
                              int nranks, unsigned long long header, uint32_t* err, const float* r,
                              RnormRec* rec, float* out, hipStream_t s);
// `nwords` words of a device record behind `header` into a gather slot, the rest of the slot zero
// (the statistics' record on its way to the exchange)
hipError_t launch_record_pack(const void* src, int nwords, unsigned long long header,
                              unsigned long long* slot, hipStream_t s);

// ---- wk_net.hip
// the general networks' kernels (wk_net.hip; NetworkKernels = 1).  nets: device copy of
// {critic, actor}; act_rows: net_act_rows of the two
enum : int { NET_MAX_BLOCKS = 1024 };  // gradient blocks (one slab each) per minibatch
hipError_t configure_net_kernels();
int net_act_rows(const NetDesc& critic, const NetDesc& actor);
int net_slab_floats(int np);
int net_grad_blocks(int samples);
hipError_t launch_net_policy(const EnvParams& P, const NetDesc* nets, int act_rows, const float* W,
                             float lp_const, int n, const float* obs, const int32_t* env_ids,
                             const uint32_t* steps, float* mean, float* act, float* logp, float* v,
                             hipStream_t s);
hipError_t launch_net_grad(const GradArgs& g, const NetDesc* nets, int act_rows, int np, hipStream_t s);
int net_stats_blocks(int rows);
hipError_t launch_net_stats(const StatsArgs& a, const NetDesc* nets, int act_rows, bool log_std,
                            hipStream_t s);
// Xavier-normal init of W[0..np), both kernel families (a built-in context: the default strings')
hipError_t launch_xavier(float* W, uint64_t seed, const NetDesc& critic, const NetDesc& actor, int np,
                         hipStream_t s);

// ---- wk_episodes.hip
// data collection: per-episode totals of a recorded rollout appended to the device log;
// layout == wk_episode_rec (include/wk_api.h)
struct EpisodeRecDev {
  float total_reward;
  int32_t env;
  int32_t length;
  uint32_t step;
};
struct EpisodeArgs {
  int n, T, env_offset;
  uint32_t step0;             // rollout env-steps taken before this one
  const float* rewards;      // [T][n]
  const uint8_t* dones;      // [T][n]
  double* acc;               // [n] running episode reward (carried across rollouts)
  int32_t* len;              // [n] running episode length
  float2* scratch;           // [T][n] (total, length bits), written where done
  uint32_t* row_cnt;         // [episode_count_cells(n, T)], zero on entry and exit
  uint64_t* log_count;       // records appended so far (may exceed cap: dropped)
  uint64_t cap;
  EpisodeRecDev* log;
};
hipError_t launch_episode_log(const EpisodeArgs& a, hipStream_t s);
int episode_count_cells(int n, int T);
hipError_t launch_episode_reset(int n, const uint8_t* mask, double* acc, int32_t* len,
                                hipStream_t s);

// ---- wk_eval.hip
// Policy evaluation (wk_evaluate; wk_eval.hip).  The accounting kernel k_eval_step runs after
// every env-step of the evaluation's private walker records, on SoA per-walker state; k_eval_fold
// and k_eval_finish fold the [episodes][n] records with the discipline of wk_stats.h (integers and
// doubles, lanes in lane order, waves in wave order, blocks in block order, no floating-point
// atomics).  EvalRecDev's layout == wk_eval_rec (include/wk_api.h).
struct EvalRecDev {
  float total_reward;
  int32_t length;
  float distance;
  float final_x;
  int32_t end;
  int32_t env;
};
enum : int { EVAL_FELL = 0, EVAL_TIME_LIMIT = 1, EVAL_SUCCESS = 2, EVAL_UNFINISHED = 3 };
struct EvalArgs {
  int n, episodes, env_offset, max_timesteps;
  // one env-step's physics outputs (the scratch row)
  const float* rew;          // [n]
  const uint8_t* done;       // [n]
  const float* pos;          // [n][2] torso position after the step, before any auto-reset
  // per-walker running episode: reward sum, length, best x, episode index (== episodes: finished)
  double* acc;               // [n]
  int32_t* len;              // [n]
  float* best;               // [n]
  int32_t* epi;              // [n]
  EvalRecDev* recs;          // [episodes][n]
  uint32_t* running;         // walkers that still have an episode to finish
};
// the fold's record: EVAL_FIELDS 64-bit words -- counts and the length sum as integers, the sums
// as doubles, then the extrema (a NaN reward stays in its minimum and maximum) and the fault OR
enum : int {
  EF_DONE = 0, EF_UNFIN, EF_FELL, EF_TIMED, EF_SUCC, EF_LEN,   // integer sums
  EF_R, EF_RR, EF_DIST,                                        // double sums
  EF_RMIN, EF_RMAX, EF_DMAX,                                   // double extrema
  EF_LMIN, EF_LMAX,                                            // integer extrema
  EF_FAULT,                                                    // OR
  EVAL_FIELDS
};
// the fold's grid: at most EVAL_FOLD_MAX_BLOCKS blocks of EVAL_FOLD_BLOCK lanes, one lane per
// walker (its episode slots in episode order), striding over the walkers: a block tile is
// EVAL_FOLD_BLOCK walkers, one grid pass EVAL_FOLD_MAX_BLOCKS * EVAL_FOLD_BLOCK
enum : int { EVAL_FOLD_BLOCK = 256, EVAL_FOLD_MAX_BLOCKS = 64 };
int eval_fold_blocks(int n);
hipError_t launch_eval_init(const EvalArgs& a, uint32_t* rng_t, uint32_t rng_step0, uint32_t* fault,
                            hipStream_t s);
hipError_t launch_eval_step(const EvalArgs& a, hipStream_t s);
hipError_t launch_eval_fold(const EvalRecDev* recs, const uint32_t* fault, int n, int episodes,
                            unsigned long long* partial /* [blocks][EVAL_FIELDS] */,
                            unsigned long long* out /* [EVAL_FIELDS] */, hipStream_t s);

// ---- wk_order.hip
// lane order for k_env_side: episode-0 walkers first, then the post-reset ones (wk_order.hip)
int order_cells(int n);  // counters: one per tile of 1,024 slots + the swap count
hipError_t launch_walker_order(const float* st, int n, uint32_t* cnt, int32_t* order,
                               int32_t* scratch /* [2 n] */, hipStream_t s);

}  // namespace wk
