/*
 * wk_api.h -- C ABI of the MI355X-native batched bipedal-walker physics + PPO engine.
 *
 * Drop-in boundary for the reference's hot path (De-Rosa/PPO-BipedalWalker, C#).  The
 * reference has no FFI of its own; these entry points replace the managed calls that
 * sit on the path (citations are /root/reference file:line):
 *
 *   wk_create / wk_destroy     Environment ctor (Environment.cs:39-51), Walker ctor
 *                              (Walker/Walker.cs:25-46), PPOAgent ctor (PPOAgent.cs:23-37),
 *                              CreateFloor (Environment.cs:211-226)
 *   wk_step, wk_step_sampled   Environment.Update (Environment.cs:64-92): SampleActions
 *                              (PPOAgent.cs:381-398) or caller actions, Clip (:78),
 *                              Walker.TakeActions/Joint.SetTorque (Walker.cs:66-75,
 *                              Joint.cs:56-61), StepObjects (Environment.cs:126-143:
 *                              Joint.Step Joint.cs:31-41 + IObject.Update Objects/IObject.cs:9
 *                              -> RigidBody.Step Bodies/RigidBody.cs:54-61), Walker.Update
 *                              (Walker.cs:49-54), CalculateReward (Environment.cs:148-154),
 *                              terminal (:106-117), GetState (Walker.cs:132-152),
 *                              auto Reset (Environment.cs:167-180)
 *   wk_reset                   Environment.Reset / Walker.Reset (Environment.cs:167-173,
 *                              Walker.cs:212-223)
 *   wk_set_materials           Walker._material : IMaterial (Walker.cs:17,30; Materials/<Name>.cs)
 *   wk_get_body_view           RigidBody.GetVectors/GetCentroid/... for Renderer and
 *                              ConsoleRenderer (Bodies/RigidBody.cs:191-261)
 *   wk_render, _device, _states Environment.RenderObjects (Environment.cs:189-208) as RGBA frames
 *                              of any list of walkers: RenderRigidObject, RenderJoints
 *                              (Rendering/Renderer.cs:90-108), GetJointColors (Walker.cs:86-99)
 *   wk_policy_sample           PPOAgent.SampleActions (PPOAgent.cs:381-398)
 *   wk_value                   PPOAgent.GetValueEstimate (PPOAgent.cs:350-364)
 *   wk_rollout                 Environment.Update x horizon with Trajectory recording
 *                              (Environment.cs:71-89, Trajectory.cs:7-50) + CalculateValues
 *                              (PPOAgent.cs:175-189)
 *   wk_ppo_update              PPOAgent.Train(Trajectory) (PPOAgent.cs:147-172): CreateBatches
 *                              (:501-540), Train(Batch) (:218-346), NeuralNetwork.Optimise /
 *                              DenseLayer.Adam (NeuralNetwork.cs:85-91, DenseLayer.cs:125-159)
 *   wk_train_batch             PPOAgent.Train(Batch) on caller data (parity entry)
 *   wk_get/set_weights         NeuralNetwork.Save/Load (NeuralNetwork.cs:94-115,159-176),
 *                              flat fp32, critic layers then actor layers, each W (out x in,
 *                              row-major) then B -- the .weights order (DenseLayer.cs:73-79)
 *   wk_comm_*                  (new) RCCL all-reduce of policy gradients across GPUs
 *
 * Conventions: every call returns 0 on success or a negative wk_status; the text is
 * in wk_last_error(ctx).  The C# side forwards it to ErrorLogger.LogError and
 * continues (the reference's log-and-continue convention, Rendering/ErrorLogger.cs:42-78).
 * Per-env soft faults (non-finite state, skipped PPO samples) are reported as bitmasks,
 * never as errors.  Host arrays are caller-owned, borrowed for the call and copied;
 * *_device variants take device pointers on the context's stream.  A context is not
 * thread-safe: one host thread per context / GPU.
 */
#ifndef WK_API_H
#define WK_API_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wk_ctx wk_ctx;

enum wk_status {
  WK_OK = 0,
  WK_ERR_ARG = -1,       /* invalid argument */
  WK_ERR_HIP = -2,       /* HIP runtime error */
  WK_ERR_CONFIG = -3,    /* unsupported configuration (e.g. non-default network DSL) */
  WK_ERR_COMM = -4,      /* RCCL error */
  WK_ERR_STATE = -5      /* call order (e.g. ppo_update before rollout) */
};

/* per-env fault bits (wk_step fault[] / wk_rollout) */
enum wk_fault { WK_FAULT_NONFINITE = 1u, WK_FAULT_SKIPPED_SAMPLE = 2u };

/* materials: Materials/<Name>.cs */
enum wk_material {
  WK_MAT_CARPET = 0, WK_MAT_ICE = 1, WK_MAT_RUBBER = 2, WK_MAT_METAL = 3, WK_MAT_WOOD = 4,
  WK_MAT_PAPER = 5, WK_MAT_TITANIUM = 6, WK_MAT_SUPERRUBBER = 7
};

/* Hyperparameters (Walker/PPO/Hyperparameters.cs:80-121): same names and defaults.
 * Batched extensions are marked (new). */
typedef struct wk_config {
  int GameSpeed;            /* 1 (UI only; ignored) */
  int Iterations;           /* 50 physics substeps per env-step */
  int MaxTimesteps;         /* 1000 */
  int RoughFloor;           /* 0; 1: CreateRoughFloor's 10 static segments with a per-walker
                               Philox terrain (every mapping) */
  int Epochs;               /* 5 */
  int BatchSize;            /* 64 */
  int UseGAE;               /* 0 */
  int NormalizeAdvantages;  /* 0 */
  float Gamma;              /* 0.9 */
  float Lambda;             /* 0.95; takes effect with ReturnsMode = 1 only: the reference never
                               chains its GAE (PPOAgent.cs:414-434), and ReturnsMode 0 restates it */
  float Epsilon;            /* 0.3 */
  float LogStandardDeviation; /* -1 */
  float Alpha;              /* 1e-3 */
  float Beta1;              /* 0.9 */
  float Beta2;              /* 0.999 */
  float AdamEpsilon;        /* 1e-8 */
  const char* CriticNeuralNetwork; /* NULL or "Input |64| (LeakyReLU) |1| Output" */
  const char* ActorNeuralNetwork;  /* NULL or "Input |64| (LeakyReLU) |64| (LeakyReLU) |4| (TanH) Output" */
  float DeltaTime;          /* MonoGame fixed step, (float)(166667 ticks / 1e7) */
  /* (new) batched extensions */
  int Horizon;              /* rollout horizon T_h of the device trajectory buffer (64) */
  int Minibatch;            /* local minibatch M for wk_ppo_update (0 -> BatchSize) */
  int MinibatchGlobal;      /* divisor of dV/dmu = global minibatch (0 -> Minibatch * nranks) */
  int EnvOffset;            /* global id of this context's env 0 (Philox streams) */
  int RandomizeStart;       /* 1: env e starts at x + 200*u_e (BASELINE config 2) */
  int RandomizeMaterial;    /* 1: env material in {Ice, Rubber, Carpet} (config 5) */
  int LanesPerWalker;       /* physics kernel mapping (all bit-exact): 2 = a lane pair per
                               walker, left / right leg chains in parallel; 4 = two lanes per
                               leg (SAT axes and contact faces split; for shards of at most
                               one wave per SIMD); 16 = SAT axes over a 16-lane row; 1 = one
                               walker per lane; 0 = auto (4 up to 16,384 walkers, else 2) */
  int NetworkKernels;       /* 0: the built-in kernels, default network strings only (any other
                               valid string is WK_ERR_CONFIG); 1: the general kernels, any valid
                               network string within the limits below, the default strings
                               included.  Limits (WK_ERR_CONFIG before a device is touched): per
                               network at most 8 layers (dense and activation together), at
                               most 4 dense layers, every width in 1..128.  The strings are
                               copied at wk_create.  One GPU (wk_comm_records refuses such a
                               context too): the multi-GPU gradient exchange
                               (wk_comm_init, wk_comm_init_host, wk_comm_ipc_handle,
                               wk_comm_init_ipc) returns WK_ERR_CONFIG on such a context.  Not
                               part of the JSON document */
  int ReturnsMode;          /* 0: the reference's returns / advantages (PPOAgent.cs:414-498): the GAE
                               chain is never carried (every advantage is the one-step TD error,
                               Lambda unused) and every reverse scan starts from 0, at a horizon
                               cut as at an episode end.  1: the standard estimators -- chained
                               GAE(Lambda), and the scan starts from the critic's value of each
                               walker's observation after the last recorded step (the bootstrap
                               values, wk_get / wk_set_bootstrap_values); a terminal step still
                               resets the scan to 0, an episode ended by MaxTimesteps included.
                               Anything else is WK_ERR_CONFIG.  Not part of the JSON document */
  float TargetKL;           /* 0 (default): off -- wk_ppo_update launches what it always did and stays
                               asynchronous.  > 0: after every epoch of wk_ppo_update, the last
                               included, the pass of wk_policy_stats runs over the whole trajectory
                               buffer and its record is copied to the host (one stream
                               synchronise per epoch); when its kl > TargetKL (strict; a NaN never
                               stops) the remaining epochs are not run.  wk_update_stats_get
                               returns the last check.  Negative or non-finite is WK_ERR_CONFIG
                               before a device is touched.  One GPU, or any number with
                               wk_comm_records: ranks deciding on their own shards would desert
                               each other mid-exchange, so without that call wk_comm_init and
                               wk_comm_init_host return WK_ERR_CONFIG on such a context (after it
                               every rank decides on the ranks' summed record);
                               wk_comm_ipc_handle and wk_comm_init_ipc always do.  Not part of the
                               JSON document */
  float MaxGradNorm;        /* 0 (default): off -- every minibatch launches what it always did.  > 0:
                               per-network gradient-norm clipping in every Adam step (wk_ppo_update,
                               wk_train_batch with apply_adam).  Critic = parameters [0, n_critic)
                               of the flat vector, actor the rest (wk_num_params); per network, on
                               the fp32 gradient Adam would have used (with a communicator: the
                               sum over the ranks, so every rank scales alike): norm = sqrt(sum
                               (double)g^2), coef = MaxGradNorm / (norm + 1e-6) in double, and the
                               gradient is multiplied by (float)coef when norm is finite and coef
                               < 1 (one fp32 product per parameter), else used as it is -- a
                               non-finite norm is counted and not scaled.  +inf measures only.
                               The minibatch tail becomes ordered reduction, then one launch
                               that forms the norms and applies Adam; the gradient buffer,
                               grads_out, the loss log and the diagnostics keep the unclipped
                               values.  wk_grad_norms_get returns the record.  Negative or NaN is
                               WK_ERR_CONFIG before a device is touched.  Works on both kernel
                               families, with wk_comm_init and wk_comm_init_host; the IPC exchange
                               fuses reduction, exchange and Adam in one launch, so
                               wk_comm_ipc_handle and wk_comm_init_ipc return WK_ERR_CONFIG on
                               such a context.  Not part of the JSON document */
  int LearnLogStd;          /* 0 (default): the policy's log-std is the constant LogStandardDeviation
                               (or what wk_set_log_std last set); wk_ppo_update launches what it
                               always did and stays asynchronous.  1: the one scalar log-std s,
                               shared by the four action dimensions, is trained.  After every
                               epoch's minibatches of wk_ppo_update, the last epoch included, the
                               pass of wk_log_std_gradient runs over the whole trajectory buffer
                               and its record is copied to the host (one stream synchronise per
                               epoch: every kernel takes std by value at launch); the host takes
                               one Adam step on s in double (Beta1, Beta2, AdamEpsilon widened;
                               learning rate LogStdAlpha, or the context's current Alpha when that
                               is 0) on grad = grad_surrogate - EntropyCoef, rounds s to float and
                               clamps it to [LogStdMin, LogStdMax].  A non-finite gradient or a
                               pass with no counted row takes no step.  Every later launch uses
                               the new value: the next epoch, wk_rollout, wk_policy_sample,
                               wk_step_sampled, wk_policy_stats, wk_evaluate; the trajectory's
                               recorded log-densities stay the old policy's.  With TargetKL > 0
                               the same pass yields that check's record (one pass per epoch; the
                               order is pass, log-std step, stop decision).  MaxGradNorm does not
                               touch s.  One GPU, or any number with wk_comm_records, like
                               TargetKL: without that call the wk_comm_* initialisers return
                               WK_ERR_CONFIG on such a context (after it every rank steps s on the
                               ranks' summed record).  Anything but 0 or 1 is
                               WK_ERR_CONFIG.  Not part of the JSON document, like the four below */
  float LogStdAlpha;        /* 0 (default): the log-std step uses the context's current Alpha
                               (wk_set_learning_rate).  > 0: its own learning rate.  Negative or
                               non-finite is WK_ERR_CONFIG */
  float EntropyCoef;        /* 0 (default).  The loss is -mean(surrogate) - EntropyCoef H with H = s +
                               ln(2 pi e) / 2, the Gaussian's entropy per dimension, so the bonus
                               adds -EntropyCoef to the gradient by s.  Finite and >= 0; > 0 with
                               LearnLogStd = 0 is WK_ERR_CONFIG (with a fixed std the bonus is a
                               constant) */
  float LogStdMin;          /* -4 */
  float LogStdMax;          /* 1.  Checked only when LearnLogStd = 1: -5 < LogStdMin <=
                               LogStandardDeviation <= LogStdMax < 5, else WK_ERR_CONFIG */
} wk_config;

/* The host-only fields of the reference's JSON configuration (SerializableHyperparameters,
 * Hyperparameters.cs:11-77), plus storage for the network DSL strings that
 * wk_config_from_json points wk_config at.  Not used by the kernels. */
typedef struct wk_host_settings {
  int CollectData;                /* 1 */
  int SaveWeights;                /* 1 */
  char CriticNeuralNetwork[256];  /* "Input |64| (LeakyReLU) |1| Output" */
  char ActorNeuralNetwork[256];   /* "Input |64| (LeakyReLU) |64| (LeakyReLU) |4| (TanH) Output" */
  char CriticWeightFileName[256]; /* "critic" */
  char ActorWeightFileName[256];  /* "actor" */
  char FilePath[1024];            /* AppDomain BaseDirectory: the executable's directory + "/" */
} wk_host_settings;

/* canonical per-env state dump: WK_STATE_FLOATS floats per env (identical layout to
 * the oracle's orc_env_dump).  Body b in {LLL, LLU, BODY, RLL, RLU} at b*20:
 * verts x0,y0..x5,y5 (BODY uses 5), centroid x,y, v x,y, w, angle, collided, pad. */
enum {
  WK_STATE_FLOATS = 112, WK_ST_TORQUE = 100, WK_ST_POS = 104, WK_ST_PREV = 106,
  WK_ST_STEPS = 108, WK_ST_POSTRESET = 109, WK_ST_TERMINAL = 110, WK_ST_EPISODES = 111,
  WK_NPARAM_CRITIC = 897, WK_NPARAM_ACTOR = 5252, WK_NPARAM = 6149, WK_OBS = 12, WK_ACT = 4,
  WK_NPAIRS = 9
};

/* per-substep pair bookkeeping (bit-exact parity outputs).  Canonical
 * pair index: 0 (LLL,LLU) 1 (LLL,FLOOR) 2 (LLU,LLL) 3 (LLU,FLOOR) 4 (BODY,FLOOR)
 * 5 (RLL,RLU) 6 (RLL,FLOOR) 7 (RLU,RLL) 8 (RLU,FLOOR). */
typedef struct wk_pair_trace {
  uint8_t aabb_hit[WK_NPAIRS];
  uint8_t sat_hit[WK_NPAIRS];
  uint8_t n_contacts[WK_NPAIRS];
  uint8_t pad[5];
  float normal[WK_NPAIRS][2];
  float depth[WK_NPAIRS];
  float contact[WK_NPAIRS][2][2]; /* contact points (n_contacts valid) */
  float impulse[WK_NPAIRS][2];    /* normal and friction impulse */
  float joint_depth[4];           /* Joint.Step gap per joint (0 if < 0.1) */
  float joint_impulse[4];
} wk_pair_trace;

/* one body of one env, for Renderer.RenderRigidObject / ConsoleRenderer */
typedef struct wk_body_view {
  int n_vertices;
  float vertices[6][2];
  float centroid[2];
  float linear_velocity[2];
  float angular_velocity;
  float angle;
  int collided;
  int is_static;
} wk_body_view;

/* Scene prop (extension of SURVEY 8(f) next-3): a Square / Triangle / Hexagon body built by
 * <Shape>.FromSize(material, (cx, cy), size, isStatic) (Objects/RigidBodies/Square.cs:18-31,
 * Triangle.cs:18-30, Hexagon.cs:18-33), then SmoothCorners(smooth) (Skeleton.cs:33-53; the
 * centroid keeps its FromSize value), SetLinearVelocity((vx, vy)), SetAngularVelocity(w) and
 * AddAcceleration((ax, ay)) (RigidBody.cs:143-183; gravity would be (0, 980)).  Every walker
 * gets its own copy, listed after the floor: the line a maintainer adds after CreateFloor()
 * in the Environment constructor (Environment.cs:39-51).  Walker resets keep the props. */
enum { WK_SHAPE_SQUARE = 0, WK_SHAPE_TRIANGLE = 1, WK_SHAPE_HEXAGON = 2 };
enum { WK_MAX_PROPS = 4, WK_PROP_MAXV = 24, WK_SCENE_MAX_VERTS = 32 };
typedef struct wk_prop {
  int32_t shape;      /* WK_SHAPE_* */
  int32_t smooth;     /* SmoothCorners count: vertices = 4 / 3 / 6 times 2^smooth, <= 24 */
  int32_t material;   /* 0 Carpet, 1 Ice, 2 Rubber, 3 Metal, 4 Wood, 5 Paper, 6 Titanium,
                         7 SuperRubber (Materials/<Name>.cs) */
  int32_t is_static;
  float cx, cy, size;
  float vx, vy, w;    /* initial linear / angular velocity */
  float ax, ay;       /* acceleration */
} wk_prop;

/* one scene prop of one env (Renderer.RenderRigidObject) */
typedef struct wk_prop_view {
  int n_vertices;
  float vertices[WK_PROP_MAXV][2];
  float centroid[2];
  float linear_velocity[2];
  float angular_velocity;
  float angle;
  int is_static;
} wk_prop_view;

typedef struct wk_ppo_args {
  int epochs;          /* 0 -> config Epochs */
  int minibatch;       /* 0 -> config Minibatch */
  int minibatch_global;/* 0 -> config MinibatchGlobal */
  uint32_t update_index; /* permutation key: minibatch sampling of update #k */
} wk_ppo_args;

typedef struct wk_rollout_stats {
  double reward_sum;     /* sum of rewards over the horizon, this context */
  int64_t episodes;      /* terminal steps in the horizon */
  int64_t env_steps;     /* n_env * horizon */
  uint32_t fault_or;     /* OR of per-env fault bits */
  int32_t pad;
} wk_rollout_stats;

/* What the current actor and critic make of the trajectory buffer (wk_policy_stats), and the
 * last per-epoch check of a TargetKL > 0 update (wk_update_stats_get).  Per (row, action
 * dimension) entry, exactly as the gradient kernels define them: mean = tanhf(z3), lp = lp_const -
 * ((act - mean) / std)^2 / 2 and ratio = expf(lp - logp_old) in fp32, the clip bounds 1 +- Epsilon
 * in fp32.  A row is skipped, and leaves every statistic untouched, exactly when
 * expf(logp_old) == 0 in any of its four dimensions (the gradient kernels' skip rule).  d = lp -
 * logp_old is the fp32 difference; the sums continue in double.  With no counted row every mean
 * and ratio_max are NaN; non-finite inputs of counted rows propagate. */
typedef struct wk_ppo_stats {
  int64_t samples;            /* trajectory rows counted */
  int64_t skipped;            /* rows the skip rule drops */
  double kl;                  /* mean over counted entries of expm1(d) - d (>= 0) */
  double kl_k1;               /* mean of -d */
  double clip_fraction;       /* share of entries with ratio > 1 + Epsilon or < 1 - Epsilon */
  double ratio_max;           /* largest ratio among counted entries */
  double surrogate;           /* mean of min(ratio * adv, clip(ratio) * adv), the fp32 products */
  double value_loss;          /* mean over counted rows of (V_new - ret)^2 */
  double explained_variance;  /* 1 - Var(ret - V_new) / Var(ret), population variances over the
                                 counted rows; NaN when Var(ret) is 0 (not above the rounding of
                                 its own sums) */
  int32_t epochs_run;         /* wk_update_stats_get only; 0 from wk_policy_stats */
  int32_t stopped_early;      /* wk_update_stats_get only: 1 when fewer epochs ran than asked */
} wk_ppo_stats;

/* The derivative of the clipped surrogate by the policy's scalar log-std s over the trajectory
 * buffer (wk_log_std_gradient; the pass a LearnLogStd = 1 update runs after every epoch).  Per
 * counted (row, dimension) entry, in fp32 as wk_ppo_stats and the gradient kernels form them:
 * zz = ((act - mean) / std)^2, lp = lp_const - zz / 2, rr = expf(lp - logp_old), w = rr (partA +
 * partB partC) the gradient kernels' selection of d surrogate / d lp; d lp / d s = zz - 1, so the
 * entry's term is (double)w ((double)zz - 1).  Sums in double with the ordered fold of
 * wk_policy_stats (no atomics: the same inputs give the same bytes); the host divides.  With no
 * counted row the means are NaN; non-finite inputs of counted rows propagate. */
typedef struct wk_log_std_grad {
  int64_t samples, skipped; /* trajectory rows counted / dropped by the skip rule */
  double grad_surrogate;    /* -mean over counted entries of w (zz - 1): d (-mean surrogate) / d s */
  double grad;              /* grad_surrogate - EntropyCoef */
  double z2_mean;           /* mean zz: 1 when std matches the actions' spread about the current mean */
} wk_log_std_grad;

/* The policy's log-std and the state of its Adam step (wk_get_log_std). */
typedef struct wk_log_std_state {
  float log_std, std;       /* current: s and expf(s), as every kernel launch takes them */
  int32_t t, pad;           /* Adam step count of s */
  double m, v;              /* its moments */
  double entropy;           /* per dimension: log_std + 0.5 ln(2 pi e), double from the float */
  double grad_last;         /* the gradient of the last wk_ppo_update's last step */
  int64_t steps, clamped, nonfinite; /* of the last wk_ppo_update: steps taken, steps the clamp
                               changed, passes whose gradient was not finite (no step) */
} wk_log_std_state;

/* The gradient norms of a MaxGradNorm > 0 context's Adam steps (wk_grad_norms_get), index 0 the
 * critic, 1 the actor.  The device record is cleared at the start of every wk_ppo_update,
 * wk_train_batch and wk_minibatch_gradient, so it describes the last such call.  The sum of
 * squares has a fixed association that does not depend on the grid: the same inputs give the same
 * bytes. */
typedef struct wk_grad_norms {
  int64_t steps;          /* Adam steps covered */
  int64_t clipped[2];     /* steps whose gradient was scaled (scale < 1) */
  int64_t nonfinite[2];   /* steps whose norm was not finite (not scaled) */
  double norm_last[2];    /* the last step's norms */
  double norm_max[2];     /* the largest norm; a NaN is ignored */
  double norm_sum[2];     /* the sum of the finite norms */
  float scale_last[2];    /* the last step's factors (1: not scaled) */
  int32_t pad[2];
} wk_grad_norms;

/* Reward normalisation (wk_reward_norm_*): the rewards the returns kernels read are scaled by the
 * running standard deviation of the walkers' discounted returns, VecNormalize's reward scaling in
 * a per-rollout form.  Switched on per context at run time, not part of wk_config. */
typedef struct wk_reward_norm_args {
  int32_t enable;   /* 0: off (returns read the raw rewards, as before); 1: on */
  int32_t frozen;   /* 1: scale with the statistics as they are; update neither them nor acc */
  float clip;       /* scaled rewards are clamped to [-clip, clip]; > 0, +inf = no clamp; default 10 */
  float epsilon;    /* added to the variance; finite, >= 0; default 1e-8 */
} wk_reward_norm_args;

typedef struct wk_reward_norm {
  int64_t count;            /* discounted-return samples in the running statistics */
  double mean, m2, var;     /* running mean, sum of squared deviations, m2 / count (0 when count is 0) */
  float scale;              /* the factor the last pass used; 1 before any */
  float clip, epsilon;
  int32_t enabled, frozen, pad;
  int64_t rows, clipped, nonfinite; /* of the last pass: rows scaled, rows the clamp changed,
                                       samples left out of the statistics */
} wk_reward_norm;

/* one finished episode (data collection) */
typedef struct wk_episode_rec {
  float total_reward;  /* (float) of the double sum of its rewards, like Enumerable.Sum */
  int32_t env;         /* global walker id (EnvOffset + index) */
  int32_t length;      /* env-steps in the episode */
  uint32_t step;       /* env-step it finished at, counted over this context's wk_rollout
                          calls (equal across ranks stepping in lockstep) */
} wk_episode_rec;

/* kernel timing (HIP events on the context's stream), cumulative since last reset */
typedef struct wk_profile {
  double physics_ms;   int64_t physics_launches;  int64_t physics_env_steps;
  double grad_ms;      int64_t grad_launches;
  double reduce_ms;    int64_t reduce_launches;
  double adam_ms;      int64_t adam_launches;
  double allreduce_ms; int64_t allreduce_calls;
  double returns_ms;   int64_t returns_launches;
  double update_ms;    int64_t update_calls;     /* whole wk_ppo_update calls */
} wk_profile;

void wk_config_defaults(wk_config* cfg);
const char* wk_version(void);

int wk_create(const wk_config* cfg, int device, int n_env, uint64_t seed, wk_ctx** out);
int wk_destroy(wk_ctx* ctx);
const char* wk_last_error(const wk_ctx* ctx); /* ctx may be NULL (create errors) */
int wk_sync(wk_ctx* ctx);
int wk_num_envs(const wk_ctx* ctx);

/* environment */
int wk_reset(wk_ctx* ctx, const uint8_t* mask /* n_env or NULL = all */);
int wk_set_materials(wk_ctx* ctx, const int32_t* mat_id /* n_env */);
/* start offsets (applied at each walker's next reset); on the rough floor the split mappings'
   lane order (walkers sorted by offset, results unaffected) is rebuilt from them */
int wk_set_offsets(wk_ctx* ctx, const float* dx /* n_env; start x = 125 + dx */);
int wk_step(wk_ctx* ctx, const float* actions_or_null /* k*n_env*4, unclipped */, int k_steps,
            float* obs /* k*n_env*12 or NULL */, float* reward /* k*n_env or NULL */,
            uint8_t* done /* k*n_env or NULL */, uint32_t* fault /* n_env or NULL */);
/* Environment.Update with the agent's own sampling, returning what Environment.cs:70-89
 * records in the Trajectory: for each of k env-steps and walkers, the state observed before
 * the step (_trajectory.States, :73), the sampled UNCLIPPED action (Walker.GetActions ->
 * PPOAgent.SampleActions, :74 / PPOAgent.cs:381-398; recorded at :86), its per-dimension
 * log-probability (:74, :87), the reward (:88) and terminal flag, the critic value of the
 * state (GetValueEstimate, PPOAgent.cs:447-456), the next state (post-reset after a
 * terminal step) and the torso position after the step, BEFORE any auto-reset
 * (Walker.GetPosition as Step reads it for _bestDistance, Environment.cs:113-119).  Any
 * output may be NULL.  Layouts [k][n_env][...]. */
int wk_step_sampled(wk_ctx* ctx, int k_steps, float* states /* k*n*12 */,
                    float* actions /* k*n*4 */, float* logp /* k*n*4 */,
                    float* values /* k*n */, float* reward /* k*n */, uint8_t* done /* k*n */,
                    float* next_obs /* k*n*12 */, uint32_t* fault /* n */,
                    float* position /* k*n*2 */);
int wk_step_device(wk_ctx* ctx, const float* d_actions_or_null, int k_steps, float* d_obs,
                   float* d_reward, uint8_t* d_done, uint32_t* d_fault);
/* one env-step with per-substep pair bookkeeping: trace[n_env * Iterations] */
int wk_step_traced(wk_ctx* ctx, const float* actions /* n_env*4 */, wk_pair_trace* trace);
int wk_get_obs(wk_ctx* ctx, float* obs /* n_env*12 */);
int wk_get_state(wk_ctx* ctx, float* state /* n_env*WK_STATE_FLOATS */);
/* wk_set_state (and wk_checkpoint_load's walker records) refuse, with WK_ERR_ARG and the walker
 * and body in wk_last_error, a state whose leg segments are not rigid walker poles: the kernels
 * project a pole onto its own edge axes over fixed vertex groups (exact for Pole.FromSize's
 * shape, Pole.cs:18-34, moved and rotated rigidly), so every vertex must stay >= 3.5 px outside
 * the groups it is left out of (the template has 7.5 px).  Non-finite poles are not checked.
 * wk_check_state runs the same check on host memory (no context, no device): WK_OK, or
 * WK_ERR_ARG with the first failing walker and body (record body index) in *bad_env / *bad_body. */
int wk_set_state(wk_ctx* ctx, const float* state /* n_env*WK_STATE_FLOATS */);
int wk_check_state(const float* state, int n_env, int* bad_env, int* bad_body);
/* The reference's per-body call shape (new entry points for a host that keeps
 * Environment.StepObjects, Environment.cs:126-143): per substep it calls Joint.Step on the 4 joints
 * (Joint.cs:31-41) and IObject.Update (Objects/IObject.cs:9) on every body of its list, after
 * Walker.TakeActions (Walker.cs:66-75).  The GPU resolves a whole env-step (every substep, joint
 * and body of every walker of the context) in one launch, so:
 *   wk_take_actions   stores walker env's 4 torques (unclipped; clipped in-kernel) for the next
 *                     frame; a walker given none keeps its current torques (no kick)
 *   wk_object_update  the frame's FIRST call runs one env-step of every walker with those torques
 *                     (returns 1); the other list_count * Iterations - 1 calls of the frame are
 *                     counted and return 0 (deltaTime: the caller's substep; the context's
 *                     DeltaTime is used)
 *   wk_joint_step     resolved inside the step: a no-op (returns 0)
 *   wk_body_order     walker env's body list now: part ids (0 LLL, 1 LLU, 2 Body, 3 RLL, 4 RLU,
 *                     5 floor / 5..14 rough-floor segments) floor last in episode 0 and first after
 *                     a reset (Walker.cs:191-234) -- at most 15 */
int wk_take_actions(wk_ctx* ctx, int env, const float* actions /* 4 */);
int wk_object_update(wk_ctx* ctx, int list_count, float delta_time);
int wk_joint_step(wk_ctx* ctx);
int wk_body_order(wk_ctx* ctx, int env, int* parts /* 15 */, int* count);
int wk_get_body_view(wk_ctx* ctx, int env, int body /* 0..4 walker, 5 floor (5..14 rough-floor segments) */,
                     wk_body_view* out);

/* policy / value */
/* Scene props for every walker (n_props <= WK_MAX_PROPS, at most WK_SCENE_MAX_VERTS vertices
 * in total; 0 removes them), each initialised as described at wk_prop.  With props the
 * env-step runs the one-lane scene kernel (LanesPerWalker 0 or 1), on either floor: with
 * RoughFloor the list is [walker, 10 segments, props] (after a reset [segments, props,
 * walker]), and props resolve against every segment. */
int wk_set_scene(wk_ctx* ctx, const wk_prop* props, int n_props);
int wk_get_prop_view(wk_ctx* ctx, int env, int prop, wk_prop_view* out);
int wk_get_weights(wk_ctx* ctx, float* params /* WK_NPARAM */);
int wk_set_weights(wk_ctx* ctx, const float* params);
int wk_get_adam(wk_ctx* ctx, float* m, float* v, int* t);
int wk_set_adam(wk_ctx* ctx, const float* m, const float* v, int t);

/* JSON configuration files (replaces Hyperparameters.SerializeJson / DeserializeJson,
 * Hyperparameters.cs:124-187, System.Text.Json default options, WriteIndented on save).
 * wk_config_to_json: NULL cfg / host = defaults; returns -(bytes needed) when cap is too
 * small.  wk_config_from_json: the document updates *cfg and *host in place (missing
 * properties keep their values); a malformed document or a value outside
 * ValidateHyperparameterValues (:189-217) returns WK_ERR_CONFIG and changes nothing;
 * otherwise returns the number of ValidateVariables (:240-290) corrections (invalid file
 * path / weights file names / network strings reset to defaults), their messages (one per
 * line) in wk_last_error(NULL).  cfg's network-string pointers are set to host's buffers.
 * No device is touched. */
void wk_host_settings_defaults(wk_host_settings* host);
int wk_config_to_json(const wk_config* cfg, const wk_host_settings* host, char* out, size_t cap);
int wk_config_from_json(const char* json, wk_config* cfg, wk_host_settings* host);
int wk_config_save_json(const char* path, const wk_config* cfg, const wk_host_settings* host);
int wk_config_load_json(const char* path, wk_config* cfg, wk_host_settings* host);

/* Weights files in the reference's text format (replaces PPOAgent.Save / Load,
 * PPOAgent.cs:192-213, over NeuralNetwork.Save / Load NeuralNetwork.cs:94-176,
 * DenseLayer.Save / Load DenseLayer.cs:55-79, Matrix.Save / Load Matrix.cs:109-153):
 * line 0 the network DSL string, then per dense layer "W <out*in row-major> B <out>",
 * floats written as .NET Core's float.ToString() (shortest round-trip, "1E-05" style).
 * Unlike the reference (which silently keeps its weights), a mismatching DSL line or a
 * malformed token is an error (WK_ERR_CONFIG / WK_ERR_ARG) and nothing is changed. */
int wk_save_weights(wk_ctx* ctx, const char* critic_path, const char* actor_path);
int wk_load_weights(wk_ctx* ctx, const char* critic_path, const char* actor_path);
/* context-free text conversion of a WK_NPARAM vector (no GPU).  wk_format_weights returns
 * -(bytes needed) when a buffer is too small. */
int wk_format_weights(const float* params, char* critic_text, size_t critic_cap,
                      char* actor_text, size_t actor_cap);
int wk_parse_weights(const char* critic_text, const char* actor_text, float* params);
/* The same for any pair of network strings (NULL: the default string), the vector holding
 * wk_net_param_count parameters: critic dense layers, then the actor's, each W (out x in,
 * row-major) then b.  WK_ERR_CONFIG for an invalid or over-limit string, or a text whose
 * line 0 is another string. */
int wk_format_weights_net(const char* critic_net, const char* actor_net, const float* params,
                          char* critic_text, size_t critic_cap, char* actor_text, size_t actor_cap);
int wk_parse_weights_net(const char* critic_net, const char* actor_net, const char* critic_text,
                         const char* actor_text, float* params);
/* Parameter counts of a pair of network strings (NULL: the default string; no GPU), and of a
 * context's networks: every parameter-shaped argument of a NetworkKernels = 1 context
 * (wk_get / set_weights, wk_get / set_adam, grads_out) holds n_critic + n_actor floats
 * instead of WK_NPARAM.  wk_net_param_count returns WK_ERR_CONFIG and a message
 * (wk_last_error(NULL)) for an invalid string or one beyond the general kernels' limits. */
int wk_net_param_count(const char* critic_net, const char* actor_net, int* n_critic, int* n_actor);
int wk_num_params(wk_ctx* ctx, int* n_critic, int* n_actor);

/* Binary checkpoint for bit-exact resume (new; the reference persists only weights):
 * weights, Adam m / v / t, every walker record, Philox step counters, start offsets,
 * materials, running episode rewards / lengths, the episode-log clock and the scene props
 * (descriptions and every walker's prop state; loading replaces the context's scene) (the episode and
 * loss logs are not included: drain them first).  Loading requires the same n_env, seed and EnvOffset; it invalidates the
 * trajectory buffer (roll out again before wk_ppo_update).
 * A NetworkKernels = 1 context writes a newer file version that also carries its two network
 * strings; loading a file written with other strings or another NetworkKernels is WK_ERR_ARG. */
int wk_checkpoint_save(wk_ctx* ctx, const char* path);
int wk_checkpoint_load(wk_ctx* ctx, const char* path);
int wk_policy_sample(wk_ctx* ctx, int n, const float* obs /* n*12 */, const int32_t* env_ids,
                     const uint32_t* steps, float* mean, float* act, float* logp);
int wk_value(wk_ctx* ctx, int n, const float* obs, float* v);

/* rollout + PPO (device-resident trajectory buffer [Horizon][n_env]) */
int wk_rollout(wk_ctx* ctx, int horizon /* <= config Horizon; 0 = Horizon */);
int wk_rollout_stats_get(wk_ctx* ctx, wk_rollout_stats* out);
int wk_get_trajectory(wk_ctx* ctx, float* states, float* actions, float* logp, float* rewards,
                      uint8_t* dones, float* values, float* returns, float* advantages);
int wk_set_trajectory(wk_ctx* ctx, int horizon, const float* states, const float* actions,
                      const float* logp, const float* rewards, const uint8_t* dones,
                      const float* values);
int wk_compute_returns(wk_ctx* ctx);
/* The bootstrap values of a ReturnsMode = 1 context: v[e] is the value the reverse scan of
 * walker e starts from, the critic's estimate of the state after the trajectory's last row (not
 * used when that row is terminal).  They belong to the trajectory buffer: wk_rollout fills them
 * with wk_value of every walker's observation after its last env-step (post-reset after a
 * terminal step), wk_set_trajectory and wk_checkpoint_load invalidate them, wk_snapshot leaves
 * them alone.  wk_set_bootstrap_values (after wk_rollout or wk_set_trajectory) replaces them and
 * marks the returns stale: the next wk_compute_returns / wk_ppo_update recomputes them.  After
 * wk_set_trajectory, wk_compute_returns, wk_ppo_update and wk_time_gradient* return WK_ERR_STATE
 * until the values are set: a host that feeds complete episodes passes zeros, one that cuts
 * episodes passes wk_value of the next observations.  Both calls are WK_ERR_STATE on a
 * ReturnsMode = 0 context, wk_get_bootstrap_values also while no valid values exist. */
int wk_get_bootstrap_values(wk_ctx* ctx, float* v /* n_env */);
int wk_set_bootstrap_values(wk_ctx* ctx, const float* v /* n_env */);
int wk_ppo_update(wk_ctx* ctx, const wk_ppo_args* args, float* critic_diag, float* actor_diag);
/* The context's current actor and critic on every row of the valid trajectory buffer (T_valid x
 * n_env, layout [t][e]): one forward-only matrix-core pass and an ordered reduction (no atomics:
 * the same inputs give the same bytes).  It uses the buffer's returns and advantages (after the
 * normalisation when NormalizeAdvantages is set) and computes them first when they are stale,
 * with wk_ppo_update's rules: WK_ERR_STATE without a trajectory, or on a ReturnsMode = 1 context
 * without bootstrap values.  The optional outputs receive the per-row fp32 log-densities
 * logp_new[t][e][4] and values values_new[t][e] of every row, skipped rows included.  No state a
 * later call can observe changes: weights, Adam, Philox counters, trajectory, whether the returns
 * count as valid, logs.  With a communicator it reports this rank's shard
 * (wk_policy_stats_global: all the ranks').
 * wk_update_stats_get: the record of the last per-epoch check of this context's last
 * wk_ppo_update, with epochs_run and stopped_early; WK_ERR_STATE when that update made no check
 * (TargetKL = 0, or no update yet). */
int wk_policy_stats(wk_ctx* ctx, wk_ppo_stats* out, float* logp_new /* T*n*4 or NULL */,
                    float* values_new /* T*n or NULL */);
int wk_update_stats_get(wk_ctx* ctx, wk_ppo_stats* out);
/* The raw sums behind wk_ppo_stats and wk_log_std_grad: the record the device passes end in and
 * the host divides, as the record exchange (wk_comm_records) gathers it.
 * wk_ppo_sums_add: the fold step, acc = acc + x -- integers add, doubles add, rmax is the larger
 * with a NaN on either side staying.  wk_ppo_stats_from_sums and wk_log_std_grad_from_sums: the
 * divisions of wk_policy_stats and wk_log_std_gradient (epochs_run and stopped_early 0).  The
 * three are host arithmetic with no context and no device; NULLs are ignored.
 * wk_policy_sums: the log-std pass once, with wk_policy_stats' state rules and errors; *local is
 * this rank's record.  A non-NULL global makes the call COLLECTIVE on a record-exchange context
 * (every rank makes it): *global is the ranks' records folded in rank order, the same bytes on
 * every rank.  A context with no communicator returns the local record as the global one; a
 * communicator without wk_comm_records is WK_ERR_STATE.  wk_policy_stats_global:
 * wk_ppo_stats_from_sums of that global record. */
typedef struct wk_ppo_sums {
  int64_t rows, skipped, clipped;  /* counted rows, skipped rows, clipped (row, dimension) entries */
  double kl, k1, surr;             /* over counted entries: expm1(d) - d, -d, the clipped surrogate */
  double sr, srr, se, see;         /* over counted rows: ret, ret^2, e = ret - V, e^2 */
  double rmax;                     /* largest ratio (-inf: none; a NaN stays) */
  double term, zz;                 /* the log-std pass's two sums: w (zz - 1) and zz */
} wk_ppo_sums;
void wk_ppo_sums_add(wk_ppo_sums* acc, const wk_ppo_sums* x);
void wk_ppo_stats_from_sums(const wk_ppo_sums* s, wk_ppo_stats* out);
void wk_log_std_grad_from_sums(const wk_ppo_sums* s, float entropy_coef, wk_log_std_grad* out);
int wk_policy_sums(wk_ctx* ctx, wk_ppo_sums* local, wk_ppo_sums* global_or_null);
int wk_policy_stats_global(wk_ctx* ctx, wk_ppo_stats* out);
/* wk_grad_norms_get: the gradient-norm record of the last wk_ppo_update / wk_train_batch of a
 * MaxGradNorm > 0 context.  It synchronises the stream (wk_ppo_update itself stays asynchronous).
 * WK_ERR_STATE on a MaxGradNorm = 0 context, or when no Adam step ran since the record was last
 * cleared; WK_ERR_ARG for NULLs.
 * wk_set_learning_rate: Alpha from the next Adam step on, on every path (a host annealing it;
 * wk_config.Alpha is otherwise copied at wk_create).  alpha must be finite and >= 0, else
 * WK_ERR_ARG and nothing changes.  Not checkpointed, like the rest of the configuration.
 * wk_get_learning_rate reads it back. */
int wk_grad_norms_get(wk_ctx* ctx, wk_grad_norms* out);
int wk_set_learning_rate(wk_ctx* ctx, float alpha);
int wk_get_learning_rate(wk_ctx* ctx, float* alpha);
/* The policy's log-std (LearnLogStd, wk_log_std_state, wk_log_std_grad).
 * wk_get_log_std: any context; on a LearnLogStd = 0 context t, m, v and the counters are 0.
 * wk_set_log_std: any context (a host annealing the noise itself uses it with LearnLogStd = 0).
 * log_std must be finite and inside (-5, 5), on a LearnLogStd = 1 context also inside [LogStdMin,
 * LogStdMax]; else WK_ERR_ARG and nothing changes.  log_std, std = expf(log_std) and the
 * log-density's constant are formed as wk_create forms them, so setting the create-time value
 * reproduces the create-time bits; every later launch uses them.  It keeps m, v and t.  On a
 * LearnLogStd = 0 context the value is configuration, like the learning rate: not checkpointed.
 * wk_set_log_std_adam: the step's moments and count.  WK_ERR_STATE on a LearnLogStd = 0 context;
 * WK_ERR_ARG for a non-finite m or v, a negative v or a negative t.
 * wk_log_std_gradient: the pass alone, on any context with a trajectory, at the current log-std
 * and weights, with wk_policy_stats' state rules and errors (stale returns are computed first;
 * WK_ERR_STATE without a trajectory).  It synchronises the stream and changes nothing a later
 * call can observe.
 * wk_snapshot saves log_std, m, v and t and restores them on a LearnLogStd = 1 context (on a
 * LearnLogStd = 0 context the value stays what wk_set_log_std made it).  A LearnLogStd = 1 context writes
 * checkpoint version 6 (log_std, t, m, v after the network section) and loads only such files;
 * a LearnLogStd = 0 context writes versions 4 / 5 byte for byte as before and refuses version 6. */
int wk_get_log_std(wk_ctx* ctx, wk_log_std_state* out);
int wk_set_log_std(wk_ctx* ctx, float log_std);
int wk_set_log_std_adam(wk_ctx* ctx, double m, double v, int t);
int wk_log_std_gradient(wk_ctx* ctx, wk_log_std_grad* out);

/* Reward normalisation (wk_reward_norm_args, wk_reward_norm).  An enabled context keeps, on the
 * device, acc[n_env] (fp32: each walker's running discounted return, carried across rollouts, 0 at
 * enable), the running (count, mean, m2) in double, the fp32 scale and a second reward buffer
 * trs[T][n]; wk_rollout stays asynchronous.
 *
 * The full pass runs inside wk_rollout after the physics and before the bootstrap values and the
 * returns (three launches, timed in wk_profile's returns slot), and alone as wk_reward_norm_update:
 *   scan    per walker e, forward over the rows t: x = r[t][e] + (acc * Gamma) in fp32 (uncontracted,
 *           as the returns kernel forms r + disc * Gamma).  A finite x is one sample -- 1, (double)x
 *           and (double)x (double)x go to the batch's count and sums -- and becomes acc; any other x
 *           is counted in `nonfinite` and zeroes acc.  A terminal row then zeroes acc.
 *   finish  mean_b = s1 / cnt_b, m2_b = max(0, s2 - s1 mean_b); merged into the running statistics
 *           in double by Chan's formula (delta = mean_b - mean, tot = count + cnt_b, mean += delta
 *           cnt_b / tot, m2 += m2_b + delta delta count cnt_b / tot, count = tot; skipped when cnt_b
 *           is 0); var = m2 / count and scale = (float)(1 / sqrt(var + (double)epsilon)), 1 when
 *           count is 0 or the result is not finite and positive.
 *   apply   trs = r * scale, one fp32 product, then clamped: |y| > clip gives copysignf(clip, y) and
 *           is counted in `clipped`.  A NaN stays NaN; +-inf clamps to +-clip.
 * The sums are ordered (no floating-point atomics): the same inputs give the same bytes.  The
 * scale already includes the rollout being scaled, so the first rollout is scaled too: a
 * per-rollout form of VecNormalize's per-step scaling.
 *
 * Only the returns kernels read trs (wk_rollout, wk_compute_returns, wk_ppo_update's stale
 * returns): returns, advantages, value targets and bootstrap values are then in scaled units.  The
 * episode log, wk_rollout_stats_get, wk_get_trajectory's rewards, wk_count_events, wk_evaluate,
 * wk_step* and the fault bits keep the raw rewards, and none of them touches acc.
 *
 * wk_reward_norm_config: NaNs, clip <= 0, a negative or non-finite epsilon, enable or frozen outside
 * 0..1 are WK_ERR_ARG and change nothing.  The first enable allocates and zeroes the state; a
 * disable keeps it for a later enable.  Every change marks the returns stale and, with a trajectory
 * in the buffer, re-runs the apply step.  One GPU, or any number with wk_comm_records: without
 * that call it is WK_ERR_CONFIG to enable on a context with a communicator, and the wk_comm_*
 * initialisers return it on an enabled context (every rank would scale by its own shard's
 * statistics).  On a record-exchange context (wk_comm_records, then wk_comm_init or
 * wk_comm_init_host) the finish step is split: every rank's batch record (count, non-finite, sum x,
 * sum x^2) is gathered, every rank folds the records in rank order and merges the fold, so all
 * ranks end the pass with the same (count, mean, m2, var, scale) bytes, `nonfinite` counts all
 * ranks' samples, and rows / clipped / acc stay this rank's.  wk_rollout and wk_reward_norm_update
 * are then COLLECTIVE calls (every rank makes them, in the same order); on an RCCL context
 * wk_rollout stays asynchronous and a header mismatch of its exchange is reported by the next
 * wk_sync, wk_reward_norm_get, wk_get_scaled_rewards, wk_policy_sums or wk_ppo_update.  A frozen
 * pass, wk_set_trajectory's apply step, wk_reward_norm_set and wk_reward_norm_set_acc exchange
 * nothing: the caller sets them alike on every rank.
 * frozen = 1 makes every pass the apply step alone.  wk_set_trajectory on an enabled context runs
 * the apply step alone with the current scale (foreign data: nothing is learned from it); a host
 * that wants it learned calls wk_reward_norm_update once afterwards (twice counts the data twice).
 * wk_reward_norm_get: any context; one never enabled reports zeros and scale 1.  It synchronises
 * the stream.  wk_reward_norm_set replaces the statistics (count >= 0, a finite mean, a finite m2 >=
 * 0, else WK_ERR_ARG) and forms the scale by the same formula on the host; the returns go stale and
 * the apply step runs again.  wk_reward_norm_set / _get_acc / _set_acc / _update and
 * wk_get_scaled_rewards are WK_ERR_STATE on a context never enabled, _update and
 * wk_get_scaled_rewards also without a trajectory.
 * wk_reset zeroes acc of the walkers it resets; wk_set_state leaves acc alone.  wk_snapshot saves
 * and restores acc, the statistics and the scale on an enabled context.  An enabled context writes
 * checkpoint version 7 -- after every earlier section the arguments, (count, mean, m2, scale) and
 * acc[n_env] -- and loads only such files; a context not enabled writes versions 4 / 5 / 6 byte for
 * byte as before and refuses version 7 (enable first). */
void wk_reward_norm_defaults(wk_reward_norm_args* args);
int wk_reward_norm_config(wk_ctx* ctx, const wk_reward_norm_args* args);
int wk_reward_norm_get(wk_ctx* ctx, wk_reward_norm* out);
int wk_reward_norm_set(wk_ctx* ctx, int64_t count, double mean, double m2);
int wk_reward_norm_get_acc(wk_ctx* ctx, float* acc /* n_env */);
int wk_reward_norm_set_acc(wk_ctx* ctx, const float* acc /* n_env */);
int wk_reward_norm_update(wk_ctx* ctx);
int wk_get_scaled_rewards(wk_ctx* ctx, float* out /* T_valid * n_env */);

/* Policy evaluation (the engine's counterpart of the console's _bestDistance and last-episode
 * average reward, Environment.cs:55-60,119): every walker of the context plays `episodes` COMPLETE
 * episodes under the current actor -- its mean action, or sampled as wk_rollout samples -- and the
 * results come back per episode and folded.
 *
 * Private state.  The evaluation steps its own copy of the walker records and its own Philox
 * counter array (allocated on first use): the records start from the template, in the body order
 * `start` names, the counters at rng_step0; start offsets and materials are the context's, and with
 * scene props it steps a private copy of the props' current state.  Nothing a later call can
 * observe changes: walker records, Philox counters, trajectory buffer (validity and bootstrap
 * values included), episode and loss logs and the running episode sums, weights, Adam, the
 * snapshot slot, the wk_profile totals, the episode-log clock.  It runs on both kernel families, is
 * not bounded by Horizon, and with a communicator it is local to the rank (no collective).
 *
 * Per env-step four launches: the observations of the private records, the policy kernel (mean or
 * act only; Philox step = the private counters), the context's own physics kernel in its
 * caller-actions mode (every mapping, the rough floor, scene props; the actions go in unclipped and
 * are clipped as for wk_step) and the accounting kernel.  A stochastic evaluation on a built-in
 * context therefore uses the standalone policy kernel: the fused rollout's distribution, not its
 * bits; on a NetworkKernels = 1 context the kernels are the rollout's own and the episodes are
 * bit-equal to wk_rollout's from the same start.
 *
 * Episode end.  The kernels expose `done`, not Walker.Terminal, so the kind is derived from what
 * the physics emits: final_x > 900.0f is WK_EVAL_SUCCESS (Environment.cs:113-117), else length >
 * MaxTimesteps is WK_EVAL_TIME_LIMIT, else WK_EVAL_FELL -- a fall on the very step of the limit is
 * reported as WK_EVAL_TIME_LIMIT.  distance starts at -inf and takes x where x > distance, so a NaN
 * x is ignored.  After its last requested episode a walker's further steps are ignored.
 *
 * Stopping.  Every `poll` env-steps the host reads how many walkers are still running; the loop
 * ends at the first poll that reads none, or at max_steps.  Slots not finished by then are
 * WK_EVAL_UNFINISHED and zero otherwise; they are counted in `unfinished` and left out of every
 * statistic.  With no finished episode the means, std, min and max are NaN (the integer length_min
 * / length_max 0).  The fold is ordered (double sums, no floating-point atomics): the same records
 * give the same bytes.
 *
 * What to expect.  A deterministic evaluation on the flat floor without RandomizeStart,
 * RandomizeMaterial or RoughFloor plays n copies of one episode.  With start = 0 a deterministic
 * walker's episodes k > 0 repeat its episode 0 (every reset returns to the same state);
 * episodes > 1 is for stochastic runs.
 *
 * WK_ERR_ARG: episodes outside 0..WK_EVAL_MAX_EPISODES, start or stochastic outside 0..1, a
 * negative max_steps or poll, a NULL out. */
enum { WK_EVAL_MAX_EPISODES = 16 };
enum wk_eval_end { WK_EVAL_FELL = 0, WK_EVAL_TIME_LIMIT = 1, WK_EVAL_SUCCESS = 2, WK_EVAL_UNFINISHED = 3 };

typedef struct wk_eval_args {
  int32_t episodes;    /* complete episodes per walker, 1..WK_EVAL_MAX_EPISODES; 0 -> 1 */
  int32_t stochastic;  /* 0: action = the actor's mean; 1: sampled as wk_rollout samples (the policy kernel's act) */
  int32_t start;       /* 0: every walker starts as after wk_reset(NULL) (post-reset body order);
                          1: as at wk_create (episode-0 order) */
  int32_t max_steps;   /* env-step cap; 0 -> episodes * (MaxTimesteps + 1), within which every walker finishes */
  int32_t poll;        /* the host checks for completion every `poll` env-steps; 0 -> 32 */
  uint32_t rng_step0;  /* stochastic: Philox step of every walker's first env-step */
} wk_eval_args;

typedef struct wk_eval_rec {   /* one episode slot, layout [episode k][walker e] */
  float total_reward;  /* (float) of the double sum of its rewards, as wk_episode_rec */
  int32_t length;      /* env-steps */
  float distance;      /* largest torso x after any of its steps (before the auto-reset) */
  float final_x;       /* torso x after its last step */
  int32_t end;         /* wk_eval_end */
  int32_t env;         /* EnvOffset + e */
} wk_eval_rec;

typedef struct wk_eval_stats {
  int64_t episodes, unfinished, fell, timed_out, succeeded;  /* episodes: finished slots */
  int64_t env_steps;              /* steps_run * n_env */
  double reward_mean, reward_std /* population */, reward_min, reward_max;
  double length_mean;  int32_t length_min, length_max;
  double distance_mean, distance_max;
  uint32_t fault_or;   int32_t steps_run;
} wk_eval_stats;

int wk_evaluate(wk_ctx* ctx, const wk_eval_args* args /* NULL = defaults */, wk_eval_stats* out,
                wk_eval_rec* recs /* episodes * n_env or NULL */);
/* The evaluation's own two kernels alone, on the private block as the context's last wk_evaluate
 * left it (WK_ERR_STATE before one, and for a second timing of the same one): `reps` back-to-back launches of the fold (kernel pair) over
 * that evaluation's records, then -- the running episodes started again -- `reps` of the
 * accounting kernel on its last physics row, each burst between one HIP-event pair on the
 * context's stream (mean duration per launch, as wk_time_gradient).  Touches nothing but that
 * block. */
int wk_evaluate_time(wk_ctx* ctx, int reps, double* step_ms, double* fold_ms);

/* Frames (the engine's counterpart of Environment.RenderObjects, Environment.cs:189-208: every
 * rigid body as a closed polyline, Renderer.RenderRigidObject Rendering/Renderer.cs:90-99; the four
 * joints as squares coloured by their torque, Walker.GetJointColors Walker/Walker.cs:86-99; the
 * best-distance marker, Environment.cs:197-199).  One launch draws n_views walkers of the context
 * into RGBA frames on the device, from the records, materials, props and terrain the context
 * already holds -- a contact sheet, a film of saved states, image observations.  Windowing and
 * input stay outside the engine.
 *
 * Layout.  [view][row j][column i][R, G, B, A] bytes, A = 255 everywhere, row 0 at the top; world y
 * grows downward (the floor is at y = 900), as on the reference's screen.  Background (0, 0, 0).
 * Every byte of every view is written, so the image needs no clear.
 *
 * Transform (fp32, nothing fused or re-associated): u = (x - ox_view) * scale, v = (y - oy) *
 * scale, with ox_view = ox, or with follow ox_view = (posx - 0.5f * ((float)width / scale)) + ox,
 * posx the record's WK_ST_POS.
 *
 * Primitive.  A segment is (a, b, colour, thickness tau in pixels), a and b in pixel coordinates.
 * With d = b - a, L2 = d.x d.x + d.y d.y, c = (i + 0.5f, j + 0.5f), e = c - a, t = e.x d.x + e.y d.y
 * and cr = e.x d.y - e.y d.x, pixel (i, j) is covered exactly when L2 > 0, t >= 0, t < L2 and cr cr <
 * (0.25f tau tau) L2: a rectangle of length |d| and width tau around the segment, half-open along
 * it -- the shape of the reference's scaled 1 x 1 sprite (Renderer.cs:119-124) without its
 * sub-pixel sampling rules.  No square root, no divide.  A NaN fails every comparison, so a
 * non-finite vertex draws nothing and never faults.
 *
 * Painter's order: the covering segment with the highest index gives the colour.  In order:
 *   1. with `joints`, 16 edges: per joint k of Walker._joints (Walker.cs:182-187; 0 BODY v1 - LLU v4,
 *      1 BODY v1 - RLU v4, 2 LLU v2 - LLL v3, 3 RLU v2 - RLL v3) the square of side 3 world units
 *      about (A + B) / 2f with Renderer.DrawSquare's corners (Renderer.cs:127-135), thickness 2
 *      line_px, colour R = (int)(value 255f + 0.5f), G = 0, B = (int)((1f - value) 255f + 0.5f) with
 *      value = (1f + clamp(torque_k, -1, 1)) / 2f, a NaN torque counting as 0;
 *   2. with a marker_x that is not NaN, the Lime segment (marker_x, 500) - (marker_x, 900), thickness
 *      2 line_px;
 *   3. the floor, White: 4 edges, or with RoughFloor the 10 segments x 4 edges in segment order
 *      (wk_get_body_view's vertices; the terrain is regenerated on the device);
 *   4. LLL, LLU, BODY, RLL, RLU (6, 6, 5, 6, 6 edges, vertex k to vertex (k + 1) mod n) in the
 *      walker's material colour: Gray (128,128,128) for Carpet, Rubber, Paper and SuperRubber, Cyan
 *      (0,255,255) Ice, White Metal, SandyBrown (244,164,96) Wood, SlateGray (112,128,144) Titanium
 *      (Materials/<Name>.cs, XNA's named colours);
 *   5. the props in scene order, a static one White, a dynamic one in its material's colour.
 * Outlines have thickness line_px.  At most 16 + 1 + 40 + 29 + 32 = 118 segments per view.  The
 * order is fixed, where the reference's list order flips after a reset (wk_body_order).
 *
 * wk_render draws the context's current records of the listed walkers (repeats allowed, every view
 * independent), stream-ordered on the context's stream -- after an asynchronous wk_rollout it shows
 * the state after that rollout -- then copies the frames to the host and synchronises.
 * wk_render_device is the same without the copy and without a synchronise: d_rgba is device memory,
 * 4-byte aligned (one packed store per pixel).  The walker ids are a HOST array in every variant, so
 * every index the kernel uses has been checked; they are copied to a buffer the context keeps.
 * That copy (and wk_render_states' copy of the records) is a stream-ordered host-to-device copy
 * from the caller's pageable array: the array may be reused as soon as the call returns, and
 * the runtime is free to stage it and to wait for earlier work on the stream before returning, so
 * "no synchronise" means the call never waits for its own kernel, not that it can never block.
 * The burst scripts/render_episode.py --bench times includes this copy in every call.
 * wk_render_states draws host records (wk_get_state's layout) as if walker envs[i] had record
 * states[i]: material, terrain and props are walker envs[i]'s as they are now.  It only draws, so
 * wk_set_state's pole rule is not checked.
 * No call changes anything a later call can observe: walker records, Philox counters, trajectory
 * buffer (validity and bootstrap values included), logs, weights, Adam, the snapshot slot, the
 * reward normalisation, the wk_profile totals.  Every context: both kernel families, every
 * LanesPerWalker, RoughFloor, scene props; with a communicator it is local to the rank.
 *
 * WK_ERR_ARG, with the text in wk_last_error and nothing launched or written: a NULL pointer,
 * n_views outside 1..WK_RENDER_MAX_VIEWS, a walker id outside [0, n_env), a dimension outside
 * 1..WK_RENDER_MAX_DIM, a non-finite or non-positive scale or line_px, a non-finite ox or oy, follow
 * or joints outside 0..1, a misaligned d_rgba. */
enum { WK_RENDER_MAX_VIEWS = 4096, WK_RENDER_MAX_DIM = 2048, WK_RENDER_MAX_SEGMENTS = 160 };
typedef struct wk_render_args {
  int32_t width, height;  /* pixels, 1..WK_RENDER_MAX_DIM each; default 550 x 325 */
  float scale;            /* pixels per world unit, finite, > 0; default 0.5 */
  float ox, oy;           /* world coordinates of the image's top-left corner; default (-50, 400): with
                             the default frame a window of 1100 x 650 units, the whole flat floor */
  int32_t follow;         /* 0 (default): ox as given.  1: ox is added to (torso x - 0.5f * ((float)width / scale)) */
  float line_px;          /* thickness of body outlines in pixels, finite, > 0; default 1; joints and
                             the marker use 2 * line_px */
  float marker_x;         /* world x of the vertical Lime marker from y = 500 to y = 900; NaN (default) = none */
  int32_t joints;         /* 1 (default): draw the joint squares */
  int32_t pad;
} wk_render_args;
void wk_render_defaults(wk_render_args* args); /* no device; a NULL is ignored */
int wk_render(wk_ctx* ctx, const wk_render_args* args, const int32_t* envs /* host, n_views */, int n_views,
              uint8_t* rgba /* host, n_views*height*width*4 */);
int wk_render_device(wk_ctx* ctx, const wk_render_args* args, const int32_t* envs /* HOST */, int n_views,
                     uint8_t* d_rgba /* device */);
int wk_render_states(wk_ctx* ctx, const wk_render_args* args, const float* states /* host, n_views*WK_STATE_FLOATS */,
                     const int32_t* envs /* host */, int n_views, uint8_t* rgba /* host */);

/* Train(Batch) on caller data: B samples, divisor b_div; grads_out (optional, WK_NPARAM)
 * receives the accumulated gradient before Adam. Returns skipped-sample count in *skipped. */
int wk_train_batch(wk_ctx* ctx, int B, float b_div, const float* states, const float* actions,
                   const float* logp_old, const float* returns, const float* adv,
                   float* critic_diag, float* actor_diag, float* grads_out, int apply_adam,
                   int* skipped);
/* The same minibatch gradient as computed inside wk_ppo_update (matrix-core kernel,
 * samples summed in 16-sample MFMA blocks -- a different fp32 association than
 * Train(Batch)'s sequential loop, PPOAgent.cs:228-335); no Adam step. */
int wk_minibatch_gradient(wk_ctx* ctx, int B, float b_div, const float* states,
                          const float* actions, const float* logp_old, const float* returns,
                          const float* adv, float* critic_diag, float* actor_diag,
                          float* grads_out, int* skipped);

/* Data collection (replaces ConsoleRenderer.AddTotalEpisodeReward / AddCriticLoss /
 * AddActorLoss, ConsoleRenderer.cs:79-95, fed by PPOAgent.Train PPOAgent.cs:151,165-166,
 * and CreateDataFile :124-135).  On by default (Hyperparameters.CollectData = true): every
 * wk_rollout appends each finished episode to a device log in completion order
 * (env-step, walker) -- wk_step does not feed it -- and every wk_ppo_update appends its last minibatch's
 * (critic, actor) diagnostics.  The episode log holds n_env * Horizon records and the loss
 * log 65,536 updates; drain them at least that often (the overflow is counted in
 * *dropped).  Drains clear the logs; a cap smaller than the held count is WK_ERR_ARG. */
int wk_collect_data(wk_ctx* ctx, int on);
int wk_episode_log_count(wk_ctx* ctx, int64_t* episodes, int64_t* updates);
int wk_episode_log_drain(wk_ctx* ctx, wk_episode_rec* out, int64_t cap, int64_t* n_out,
                         int64_t* dropped);
int wk_loss_log_drain(wk_ctx* ctx, float* critic, float* actor, int64_t cap, int64_t* n_out,
                      int64_t* dropped);
/* the reference's data file: rewards / critic losses / actor losses lists, no device */
int wk_write_data_file(const char* path, const float* total_rewards, int64_t n_rewards,
                       const float* critic_losses, int64_t n_critic, const float* actor_losses,
                       int64_t n_actor);

/* multi-GPU: RCCL communicator over the ranks' contexts (one per GPU) */
int wk_comm_unique_id(uint8_t* id /* 128 bytes */);
/* The record exchange: TargetKL, LearnLogStd and reward normalisation on any number of GPUs.
 * wk_comm_records, called before the gradient exchange is initialised, declares that this
 * context's ranks will exchange their statistics records.  fn NULL: RCCL (ncclAllGather of the
 * WK_COMM_RECORD_WORDS words on the context's stream), valid only when followed by wk_comm_init;
 * otherwise the host control plane, valid only when followed by wk_comm_init_host: fn receives
 * this rank's record and must fill `all` with every rank's, in rank order (return 0).  It is the
 * counterpart of wk_host_allreduce_fn and is kept for the context's lifetime.  After the call the
 * matching initialiser accepts a context with TargetKL > 0, LearnLogStd = 1 or reward
 * normalisation enabled, and wk_reward_norm_config may enable once the communicator exists.
 * Without the call nothing changes.  WK_ERR_STATE after any wk_comm_* initialiser, for a second
 * call, and from an initialiser that does not match the declared kind; WK_ERR_CONFIG on a
 * NetworkKernels = 1 context.  The IPC exchange stays closed: wk_comm_ipc_handle and
 * wk_comm_init_ipc return WK_ERR_CONFIG on such contexts with or without the call (they fuse
 * reduction, exchange and Adam in one launch).
 * Records are gathered, not summed in flight: every rank receives every rank's record byte for
 * byte and folds them itself in rank order starting from rank 0's, so all ranks decide on the
 * same bytes (with one rank the fold is the identity).  Word 0 of a record is its header, kind <<
 * 56 | nranks << 48 | sequence (kind 1 statistics, 2 reward normalisation; sequence this context's
 * count of record exchanges); a rank whose header differs from the caller's, a non-zero return of
 * fn or a failed ncclAllGather is WK_ERR_COMM naming the first differing rank, fatal for the job
 * like a failed all-reduce, and no step is taken.
 * On such a context, once the communicator exists: wk_ppo_update gathers one record per epoch
 * (TargetKL > 0 or LearnLogStd = 1) and takes the log-std step and the stop decision from the
 * fold, which wk_update_stats_get and wk_get_log_std's grad_last then report; wk_rollout and
 * wk_reward_norm_update gather the batch record of the reward normalisation (see there).
 * NormalizeAdvantages, wk_policy_stats, wk_log_std_gradient, wk_rollout_stats_get and wk_evaluate
 * stay this rank's shard. */
enum { WK_COMM_RECORD_WORDS = 16 };            /* one record: 16 64-bit words */
typedef int wk_host_allgather_fn(const uint64_t* mine /* 16 */, uint64_t* all /* nranks*16, rank order */,
                                 void* user);
int wk_comm_records(wk_ctx* ctx, wk_host_allgather_fn* fn_or_null, void* user);
int wk_comm_init(wk_ctx* ctx, int rank, int nranks, const uint8_t* unique_id);
/* sum of host_buf over the ranks, in place, through the context's exchange: RCCL, or with
 * wk_comm_init_ipc one round of the IPC exchange (n <= 6,152 floats; ranks summed in rank order;
 * WK_ERR_COMM when a peer never publishes) -- tests, and bench.py's check of a fresh IPC mapping */
int wk_allreduce_test(wk_ctx* ctx, float* host_buf, int n);
/* The same minibatch sequence with a caller-supplied all-reduce instead of RCCL: after the
 * ordered reduction each minibatch's slab (gradient + diagnostics, n floats) is copied to the
 * host, fn must replace it in place with the sum over ranks (return 0), and it is copied back
 * before Adam.  For hosts without RCCL (MPI, a CPU control plane) and for testing the
 * multi-rank path of several processes sharing one GPU (RCCL refuses duplicate devices).
 * fn is kept for the context's lifetime (a managed caller must keep its delegate alive).  A
 * non-zero return fails this rank's wk_ppo_update with WK_ERR_COMM mid-update (no Adam step
 * for that minibatch) while the peers wait in their own all-reduce: it is fatal for the
 * whole job -- abort every rank. */
typedef int (*wk_host_allreduce_fn)(float* buf, int n, void* user);
int wk_comm_init_host(wk_ctx* ctx, int rank, int nranks, wk_host_allreduce_fn fn, void* user);
/* The one-shot exchange over peer-mapped memory instead of RCCL (ranks on one node, at most 8):
 * wk_comm_ipc_handle allocates this rank's exchange region and returns its record (the IPC
 * handle, then the PCI bus id of the rank's GPU); the caller all-gathers the records (any
 * control plane) and passes all of them, in rank order, to wk_comm_init_ipc, which maps the
 * peers' regions (WK_ERR_ARG if more than 4 ranks share one GPU: they would stall).  Per
 * minibatch one kernel publishes this rank's ordered block sum, waits (bounded: 30 s of the
 * GPU's constant clock by default; WK_XCH_TIMEOUT_S in the environment at wk_comm_init_ipc, or
 * wk_comm_set_timeout, changes it -- the ranks must stay within it of each other: a rank busy
 * elsewhere longer than that while its peers have an update queued kills the job) for every
 * peer's, sums the ranks' slabs in rank order and applies Adam -- no collective library, no host
 * round trip.  A peer that never publishes (or gave up first) fails wk_ppo_update /
 * wk_train_batch / wk_minibatch_gradient / wk_allreduce_test with WK_ERR_COMM, fatal for the
 * job as a failed all-reduce: from the failed minibatch on this rank applies no Adam step and
 * marks its flags aborted, so a late peer fails that same minibatch instead of applying it, and
 * wk_get_adam reports the steps actually applied.  The replicas may still differ after a
 * failure (a peer that read this rank's flag just before the abort, or blocks straddling the
 * bound), and the failed context stays failed (its error word and aborted flags are not cleared
 * by wk_checkpoint_load): stop the job, or on every rank destroy the context, create a new one,
 * map the exchange again (wk_comm_ipc_handle / wk_comm_init_ipc) and load a checkpoint.
 * wk_minibatch_gradient and
 * wk_train_batch(apply_adam = 0) run the exchange as well (collective calls: every rank must
 * make them), returning the sum over the ranks as on an RCCL context. */
enum { WK_IPC_HANDLE_BYTES = 128 };
int wk_comm_ipc_handle(wk_ctx* ctx, uint8_t* handle /* WK_IPC_HANDLE_BYTES */);
int wk_comm_init_ipc(wk_ctx* ctx, int rank, int nranks, const uint8_t* handles /* nranks * 128 */);
/* the IPC exchange's bounded peer wait, in seconds (0 < seconds <= 1e6) */
int wk_comm_set_timeout(wk_ctx* ctx, double seconds);
/* the context's minibatch exchange: *kind 0 none, 1 RCCL, 2 host callback, 3 IPC; *flags bit 0:
 * the IPC exchange region is uncached device memory (else coarse-grained hipMalloc memory) */
int wk_comm_info(wk_ctx* ctx, int* kind, int* flags);
/* IPC exchange timing (new; the exchange replaces the all-reduce before PPOAgent.cs:344-345's
 * Optimise): with minibatches > 0 every exchange launch of the context stamps the GPU's 100 MHz
 * constant clock per block at four points -- entry, its slab published (flag released), every
 * peer's flag seen, exit (peer slabs read, Adam stored) -- into a device ring of `minibatches`
 * launches; 0 frees the ring.  wk_comm_xch_stamps copies the last min(stamped, max_launches)
 * launches, oldest first, as stamps[(launch * blocks + block) * 4 + point] (ticks of 10 ns). */
int wk_comm_xch_profile(wk_ctx* ctx, int minibatches);
int wk_comm_xch_stamps(wk_ctx* ctx, uint64_t* stamps, int max_launches, int* launches, int* blocks);

/* profiling */
/* level 0 off; 1: HIP events around each rollout / returns pass / whole PPO update (cheap
 * enough inside a timed loop); 2: also around every gradient / reduce / all-reduce / Adam
 * launch of the update */
int wk_profile_enable(wk_ctx* ctx, int on);
int wk_profile_get(wk_ctx* ctx, wk_profile* out);
int wk_profile_reset(wk_ctx* ctx);

/* Counting replay (the flop model priced on the physics events that actually
 * happen, RigidBody.cs:66-96 / Joint.cs:31-41): steps the walkers k env-steps with the
 * actions recorded in the device trajectory (rows 0..k-1 of the last rollout; k <= its
 * horizon) through the one-lane kernel with per-lane event counters -- the same physics bit
 * for bit as the rollout when the state is the rollout's starting state (see wk_snapshot).
 * counts[WK_NEV] (added to, not cleared) receives, in order: joints past the 0.1 early-out;
 * bounding-box hits leg-leg / leg-floor / torso-floor (each runs SAT); SAT collisions
 * (contacts + MoveObjects) in the same three classes; contact resolutions with >= 1 point
 * (the impulse pair) in the same three classes; contact points; walker-substeps; env-steps;
 * auto-resets; walker env-steps with >= 1 leg-floor bounding-box hit; walker env-steps with
 * >= 1 leg-leg SAT collision. */
#define WK_NEV 16
int wk_count_events(wk_ctx* ctx, int k, uint64_t* counts);

/* Device-side snapshot of the training state: walker records, Philox step counters, weights,
 * Adam m / v / t, episode bookkeeping and scene props (not the trajectory buffer, which keeps
 * the last rollout).  op 0 saves, op 1 restores (stream-ordered device copies, no host sync); bench.py restores one before every timed iteration so
 * each measures the same regime (the throughput no longer drifts with training).
 * A wk_episode_log_drain after the save hands the saved records out, so the next restore leaves
 * an empty episode log; the running episode sums and lengths are restored either way. */
int wk_snapshot(wk_ctx* ctx, int op);

/* The update's gradient kernel alone: `reps` back-to-back launches on minibatch 0 (update 0,
 * epoch 0 of the keyed sequence; minibatch 0 = config Minibatch) of the current trajectory,
 * timed by one HIP-event pair on the context's stream -- the kernel's mean duration without
 * per-launch event overhead (bench.py's update roofline).  Writes only scratch slabs. */
int wk_time_gradient(wk_ctx* ctx, int minibatch, int reps, double* ms_per_launch);
/* The same with flags: bit 0 puts an event pair around EVERY launch (the elapsed times summed),
 * as profile level 2 times each launch of the update.  bench.py prices the update roofline on
 * the gradient kernel's in-update duration: the level-2 per-launch mean inside a real update
 * minus the per-launch event overhead (this burst with bit 0 minus the plain burst). */
int wk_time_gradient_ex(wk_ctx* ctx, int minibatch, int reps, int flags, double* ms_per_launch);

/* The rollout kernel's mapping as launched: lanes per walker (1, 2, 4 or 16), walkers per
 * wave (fewer than 64 / lanes for the sparse quad mapping), the waves that hold walkers and
 * (waves_launched, nullable) the waves the grid launches -- the split kernels launch whole
 * 4-wave blocks whose idle waves replay the last walker.  bench.py's VALU ceiling is priced on
 * the launched grid (one wave per SIMD below 1,024 waves). */
int wk_rollout_mapping(wk_ctx* ctx, int* lanes_per_walker, int* walkers_per_wave, int64_t* waves,
                       int64_t* waves_launched);

/* Which matrix-core gradient kernel the update launches for a per-GPU minibatch of `minibatch`
 * samples (0 = config Minibatch): 0 producer / consumer waves (k_ppo_grad_ws), 1 tile-parallel
 * teams (k_ppo_grad_tp, two per block), 2 the same with one team per block, 3 one wave per chunk
 * (k_ppo_grad_mfma).  By size (tp1 up to 4,096 samples, tp below 32,768, ws from there) unless
 * WK_GRAD_IMPL = ws / tp / tp1 / mf was set at wk_create.  4: the general networks' kernel
 * (k_net_grad), on every NetworkKernels = 1 context. */
int wk_grad_kernel(wk_ctx* ctx, int minibatch);

#ifdef __cplusplus
}
#endif
#endif
