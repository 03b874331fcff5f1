// NativeMethods.cs -- P/Invoke binding of libwk.so (include/wk_api.h) for the reference's C#
// host (De-Rosa/PPO-BipedalWalker, .NET >= 6).  Every entry point of the C ABI is declared
// here with the header's parameter order; every struct mirrors the header's sequential layout
// (tests/test_csharp_binding.py checks both against include/wk_api.h and the ctypes layouts,
// since no .NET SDK exists in the build container).
//
// Conventions (wk_api.h): every call returns 0 or a negative wk_status; the message is
// wk_last_error(ctx) (ctx = IntPtr.Zero for wk_create failures) and the host logs it and
// continues, as every try/catch -> ErrorLogger.LogError does in the reference.  Arrays are
// caller-owned and copied during the call; a null array is passed as null.
using System;
using System.Runtime.InteropServices;

namespace NEA.Native;

public enum WkStatus { Ok = 0, Arg = -1, Hip = -2, Config = -3, Comm = -4, State = -5 }

public enum WkMaterial { Carpet = 0, Ice = 1, Rubber = 2, Metal = 3, Wood = 4, Paper = 5, Titanium = 6, SuperRubber = 7 }

public enum WkShape { Square = 0, Triangle = 1, Hexagon = 2 }

public static class WkConst
{
    public const int StateFloats = 112, NParam = 6149, NParamCritic = 897, NParamActor = 5252;
    public const int Obs = 12, Act = 4, NPairs = 9, MaxProps = 4, PropMaxV = 24, NEvents = 16;
    public const int IpcHandleBytes = 128;  // WK_IPC_HANDLE_BYTES: IPC handle + the GPU's PCI bus id
}

// wk_config up to MaxGradNorm, its first 128 bytes: Hyperparameters.cs:80-121 names and defaults + the batched extensions.
// The library reads and writes the whole wk_config, WkConfigLogStd below, which every import takes.
[StructLayout(LayoutKind.Sequential)]
public struct WkConfig
{
    public int GameSpeed, Iterations, MaxTimesteps, RoughFloor, Epochs, BatchSize, UseGAE,
               NormalizeAdvantages;
    public float Gamma, Lambda, Epsilon, LogStandardDeviation, Alpha, Beta1, Beta2, AdamEpsilon;
    public IntPtr CriticNeuralNetwork, ActorNeuralNetwork;  // NULL = the default networks
    public float DeltaTime;
    public int Horizon, Minibatch, MinibatchGlobal, EnvOffset, RandomizeStart, RandomizeMaterial;
    // LanesPerWalker: 0 = auto (4-lane split leg pairs up to 16,384 walkers, else the 2-lane leg split), 1 / 2 / 4 / 16 lanes.
    // NetworkKernels: 0 = the built-in kernels (default network strings only), 1 = the general kernels (any valid string within the limits)
    // ReturnsMode: 0 = the reference's returns (GAE never chained, 0 at every horizon cut), 1 = chained GAE(Lambda) and the
    // critic's value at the cut (wk_get / wk_set_bootstrap_values) -- a host that trains on complete episodes passes zeros
    public int LanesPerWalker, NetworkKernels, ReturnsMode;
    // TargetKL: 0 = off, above 0 = after every epoch of wk_ppo_update the pass of wk_policy_stats runs over the trajectory buffer
    // and the remaining epochs are not run once its Kl exceeds the target (wk_update_stats_get returns the last check)
    public float TargetKL;
    // MaxGradNorm: 0 = off, above 0 = every Adam step scales the critic's and the actor's summed gradient down to that L2 norm
    // (float.PositiveInfinity measures only, wk_grad_norms_get returns the record, the IPC exchange refuses such a context)
    public float MaxGradNorm;
}

// wk_config as include/wk_api.h declares it (wk_config_defaults fills it): WkConfig's fields in WkConfig's order,
// then the five of the trained log-std
[StructLayout(LayoutKind.Sequential)]
public struct WkConfigLogStd
{
    public int GameSpeed, Iterations, MaxTimesteps, RoughFloor, Epochs, BatchSize, UseGAE,
               NormalizeAdvantages;
    public float Gamma, Lambda, Epsilon, LogStandardDeviation, Alpha, Beta1, Beta2, AdamEpsilon;
    public IntPtr CriticNeuralNetwork, ActorNeuralNetwork;  // NULL = the default networks
    public float DeltaTime;
    public int Horizon, Minibatch, MinibatchGlobal, EnvOffset, RandomizeStart, RandomizeMaterial;
    public int LanesPerWalker, NetworkKernels, ReturnsMode;
    public float TargetKL;
    public float MaxGradNorm;
    // LearnLogStd: 0 = the log-std is the constant LogStandardDeviation (or what wk_set_log_std set), 1 = after every epoch of
    // wk_ppo_update one pass over the trajectory buffer forms the clipped surrogate's derivative by the scalar log-std and the host
    // takes one Adam step on it (one stream synchronise per epoch, one GPU: the wk_comm_* initialisers refuse such a context)
    public int LearnLogStd;
    // LogStdAlpha: that step's learning rate (0 = the context's Alpha).  EntropyCoef: the entropy bonus's weight (needs LearnLogStd = 1).
    // LogStdMin / LogStdMax: the clamp after every step, -5 < LogStdMin <= LogStandardDeviation <= LogStdMax < 5
    public float LogStdAlpha, EntropyCoef, LogStdMin, LogStdMax;
}

// SerializableHyperparameters' host-only fields (Hyperparameters.cs:11-77)
[StructLayout(LayoutKind.Sequential, CharSet = CharSet.Ansi)]
public struct WkHostSettings
{
    public int CollectData, SaveWeights;
    [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string CriticNeuralNetwork;
    [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string ActorNeuralNetwork;
    [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string CriticWeightFileName;
    [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 256)] public string ActorWeightFileName;
    [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 1024)] public string FilePath;
}

// per-substep pair bookkeeping (wk_step_traced)
[StructLayout(LayoutKind.Sequential)]
public unsafe struct WkPairTrace
{
    public fixed byte AabbHit[9];
    public fixed byte SatHit[9];
    public fixed byte NContacts[9];
    public fixed byte Pad[5];
    public fixed float Normal[18];
    public fixed float Depth[9];
    public fixed float Contact[36];
    public fixed float Impulse[18];
    public fixed float JointDepth[4];
    public fixed float JointImpulse[4];
}

// one body of one walker, for Renderer.RenderRigidObject / ConsoleRenderer
[StructLayout(LayoutKind.Sequential)]
public unsafe struct WkBodyView
{
    public int NVertices;
    public fixed float Vertices[12];
    public fixed float Centroid[2];
    public fixed float LinearVelocity[2];
    public float AngularVelocity, Angle;
    public int Collided, IsStatic;
}

// Square / Triangle / Hexagon.FromSize(...).SmoothCorners(...) + velocities, acceleration
[StructLayout(LayoutKind.Sequential)]
public struct WkProp
{
    public int Shape, Smooth, Material, IsStatic;
    public float Cx, Cy, Size;
    public float Vx, Vy, W;
    public float Ax, Ay;
}

[StructLayout(LayoutKind.Sequential)]
public unsafe struct WkPropView
{
    public int NVertices;
    public fixed float Vertices[48];
    public fixed float Centroid[2];
    public fixed float LinearVelocity[2];
    public float AngularVelocity, Angle;
    public int IsStatic;
}

[StructLayout(LayoutKind.Sequential)]
public struct WkPpoArgs
{
    public int Epochs, Minibatch, MinibatchGlobal;
    public uint UpdateIndex;
}

[StructLayout(LayoutKind.Sequential)]
public struct WkRolloutStats
{
    public double RewardSum;
    public long Episodes, EnvSteps;
    public uint FaultOr;
    public int Pad;
}

// wk_policy_stats / wk_update_stats_get: the current actor and critic on the trajectory buffer
[StructLayout(LayoutKind.Sequential)]
public struct WkPpoStats
{
    public long Samples, Skipped;
    public double Kl, KlK1, ClipFraction, RatioMax, Surrogate, ValueLoss, ExplainedVariance;
    public int EpochsRun, StoppedEarly;
}

// wk_grad_norms_get: the gradient norms of a MaxGradNorm > 0 context's Adam steps, index 0 the critic, 1 the actor
[StructLayout(LayoutKind.Sequential)]
public unsafe struct WkGradNorms
{
    public long Steps;
    public fixed long Clipped[2];
    public fixed long Nonfinite[2];
    public fixed double NormLast[2];
    public fixed double NormMax[2];
    public fixed double NormSum[2];
    public fixed float ScaleLast[2];
    public fixed int Pad[2];
}

// wk_policy_sums: the raw sums the statistics passes end in, as the record exchange (wk_comm_records) gathers them
[StructLayout(LayoutKind.Sequential)]
public struct WkPpoSums
{
    public long Rows, Skipped, Clipped;
    public double Kl, K1, Surr, Sr, Srr, Se, See, Rmax;
    public double Term, Zz;
}

// wk_log_std_gradient: the clipped surrogate's derivative by the scalar log-std over the trajectory buffer, host-divided
[StructLayout(LayoutKind.Sequential)]
public struct WkLogStdGrad
{
    public long Samples, Skipped;
    public double GradSurrogate, Grad, Z2Mean;
}

// wk_get_log_std: the policy's log-std, the Adam state of the scalar and the last update's counters
[StructLayout(LayoutKind.Sequential)]
public struct WkLogStdState
{
    public float LogStd, Std;
    public int T, Pad;
    public double M, V, Entropy, GradLast;
    public long Steps, Clamped, Nonfinite;
}

// wk_reward_norm_config: Enable 1 scales the rewards the returns kernels read by the running std of the walkers' discounted
// returns (clamped to +-Clip, Epsilon added to the variance); Frozen 1 scales with the statistics as they are
[StructLayout(LayoutKind.Sequential)]
public struct WkRewardNormArgs
{
    public int Enable, Frozen;
    public float Clip, Epsilon;
}

// wk_reward_norm_get: the running statistics, the scale the last pass used, the arguments and that pass's counters
[StructLayout(LayoutKind.Sequential)]
public struct WkRewardNorm
{
    public long Count;
    public double Mean, M2, Var;
    public float Scale, Clip, Epsilon;
    public int Enabled, Frozen, Pad;
    public long Rows, Clipped, Nonfinite;
}

// wk_evaluate: complete episodes under the current actor on a private copy of the walkers
[StructLayout(LayoutKind.Sequential)]
public struct WkEvalArgs
{
    public int Episodes;    // complete episodes per walker, 1..16 (0 = 1)
    public int Stochastic;  // 0 = the actor's mean action, 1 = sampled as wk_rollout samples
    public int Start;       // 0 = as after wk_reset(NULL), 1 = as at wk_create
    public int MaxSteps;    // env-step cap (0 = Episodes * (MaxTimesteps + 1))
    public int Poll;        // completion check every Poll env-steps (0 = 32)
    public uint RngStep0;   // stochastic: Philox step of every walker's first env-step
}

// wk_render / wk_render_device / wk_render_states: the frame, the window and what to draw
// (fill it with wk_render_defaults: 550 x 325 at scale 0.5 from (-50, 400), joints on, no marker)
[StructLayout(LayoutKind.Sequential)]
public struct WkRenderArgs
{
    public int Width, Height;  // pixels, 1..2048 each
    public float Scale;        // pixels per world unit
    public float Ox, Oy;       // world coordinates of the image's top-left corner
    public int Follow;         // 1 = Ox is added to (torso x - half the window's width)
    public float Line_px;      // thickness of body outlines in pixels (joints and the marker use twice that)
    public float Marker_x;     // world x of the vertical Lime marker, NaN = none
    public int Joints;         // 1 = draw the joint squares
    public int Pad;
}

// one episode slot of wk_evaluate, layout [episode][walker], End: 0 fell, 1 time limit, 2 success, 3 unfinished
[StructLayout(LayoutKind.Sequential)]
public struct WkEvalRec
{
    public float TotalReward;
    public int Length;
    public float Distance, FinalX;
    public int End, Env;
}

[StructLayout(LayoutKind.Sequential)]
public struct WkEvalStats
{
    public long Episodes, Unfinished, Fell, TimedOut, Succeeded, EnvSteps;
    public double RewardMean, RewardStd, RewardMin, RewardMax;
    public double LengthMean;
    public int LengthMin, LengthMax;
    public double DistanceMean, DistanceMax;
    public uint FaultOr;
    public int StepsRun;
}

[StructLayout(LayoutKind.Sequential)]
public struct WkEpisodeRec
{
    public float TotalReward;
    public int Env, Length;
    public uint Step;
}

[StructLayout(LayoutKind.Sequential)]
public struct WkProfile
{
    public double PhysicsMs; public long PhysicsLaunches; public long PhysicsEnvSteps;
    public double GradMs; public long GradLaunches;
    public double ReduceMs; public long ReduceLaunches;
    public double AdamMs; public long AdamLaunches;
    public double AllreduceMs; public long AllreduceCalls;
    public double ReturnsMs; public long ReturnsLaunches;
    public double UpdateMs; public long UpdateCalls;
}

public static class Wk
{
    const string Lib = "wk";  // libwk.so next to the executable (or on LD_LIBRARY_PATH)

    [DllImport(Lib)] public static extern void wk_config_defaults(ref WkConfigLogStd cfg);
    [DllImport(Lib)] public static extern IntPtr wk_version();
    [DllImport(Lib)] public static extern int wk_create(ref WkConfigLogStd cfg, int device, int nEnv, ulong seed, out IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern IntPtr wk_last_error(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_sync(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_num_envs(IntPtr ctx);

    // environment
    [DllImport(Lib)] public static extern int wk_reset(IntPtr ctx, byte[]? mask);
    [DllImport(Lib)] public static extern int wk_set_materials(IntPtr ctx, int[] matId);
    [DllImport(Lib)] public static extern int wk_set_offsets(IntPtr ctx, float[] dx);
    [DllImport(Lib)] public static extern int wk_step(IntPtr ctx, float[]? actions, int kSteps, float[]? obs, float[]? reward, byte[]? done, uint[]? fault);
    [DllImport(Lib)] public static extern int wk_step_sampled(IntPtr ctx, int kSteps, float[]? states, float[]? actions, float[]? logp, float[]? values, float[]? reward, byte[]? done, float[]? nextObs, uint[]? fault, float[]? position);
    [DllImport(Lib)] public static extern int wk_step_device(IntPtr ctx, IntPtr dActions, int kSteps, IntPtr dObs, IntPtr dReward, IntPtr dDone, IntPtr dFault);
    [DllImport(Lib)] public static extern int wk_step_traced(IntPtr ctx, float[] actions, [Out] WkPairTrace[] trace);
    [DllImport(Lib)] public static extern int wk_get_obs(IntPtr ctx, float[] obs);
    [DllImport(Lib)] public static extern int wk_get_state(IntPtr ctx, float[] state);
    [DllImport(Lib)] public static extern int wk_set_state(IntPtr ctx, float[] state);
    [DllImport(Lib)] public static extern int wk_check_state(float[] state, int nEnv, out int badEnv, out int badBody);
    [DllImport(Lib)] public static extern int wk_take_actions(IntPtr ctx, int env, float[] actions);
    [DllImport(Lib)] public static extern int wk_object_update(IntPtr ctx, int listCount, float deltaTime);
    [DllImport(Lib)] public static extern int wk_joint_step(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_body_order(IntPtr ctx, int env, int[] parts, out int count);
    [DllImport(Lib)] public static extern int wk_get_body_view(IntPtr ctx, int env, int body, out WkBodyView view);
    [DllImport(Lib)] public static extern int wk_set_scene(IntPtr ctx, WkProp[]? props, int nProps);
    [DllImport(Lib)] public static extern int wk_get_prop_view(IntPtr ctx, int env, int prop, out WkPropView view);

    // weights, configuration, checkpoints
    [DllImport(Lib)] public static extern int wk_get_weights(IntPtr ctx, float[] p);
    [DllImport(Lib)] public static extern int wk_set_weights(IntPtr ctx, float[] p);
    [DllImport(Lib)] public static extern int wk_get_adam(IntPtr ctx, float[]? m, float[]? v, out int t);
    [DllImport(Lib)] public static extern int wk_set_adam(IntPtr ctx, float[]? m, float[]? v, int t);
    [DllImport(Lib)] public static extern void wk_host_settings_defaults(ref WkHostSettings host);
    [DllImport(Lib)] public static extern int wk_config_to_json(ref WkConfigLogStd cfg, ref WkHostSettings host, byte[] text, UIntPtr cap);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_config_from_json(string json, ref WkConfigLogStd cfg, ref WkHostSettings host);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_config_save_json(string path, ref WkConfigLogStd cfg, ref WkHostSettings host);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_config_load_json(string path, ref WkConfigLogStd cfg, ref WkHostSettings host);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_save_weights(IntPtr ctx, string criticPath, string actorPath);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_load_weights(IntPtr ctx, string criticPath, string actorPath);
    [DllImport(Lib)] public static extern int wk_format_weights(float[] p, byte[] critic, UIntPtr criticCap, byte[] actor, UIntPtr actorCap);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_parse_weights(string critic, string actor, float[] p);
    // any pair of network strings (a null string = the default one); p holds wk_net_param_count floats
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_format_weights_net(string criticNet, string actorNet, float[] p, byte[] critic, UIntPtr criticCap, byte[] actor, UIntPtr actorCap);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_parse_weights_net(string criticNet, string actorNet, string critic, string actor, float[] p);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_net_param_count(string criticNet, string actorNet, out int nCritic, out int nActor);
    [DllImport(Lib)] public static extern int wk_num_params(IntPtr ctx, out int nCritic, out int nActor);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_checkpoint_save(IntPtr ctx, string path);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_checkpoint_load(IntPtr ctx, string path);

    // agent
    [DllImport(Lib)] public static extern int wk_policy_sample(IntPtr ctx, int n, float[] obs, int[]? envIds, uint[]? steps, float[]? mean, float[]? act, float[]? logp);
    [DllImport(Lib)] public static extern int wk_value(IntPtr ctx, int n, float[] obs, float[] v);

    // rollout + PPO
    [DllImport(Lib)] public static extern int wk_rollout(IntPtr ctx, int horizon);
    [DllImport(Lib)] public static extern int wk_rollout_stats_get(IntPtr ctx, out WkRolloutStats stats);
    [DllImport(Lib)] public static extern int wk_get_trajectory(IntPtr ctx, float[]? states, float[]? actions, float[]? logp, float[]? rewards, byte[]? dones, float[]? values, float[]? returns, float[]? advantages);
    [DllImport(Lib)] public static extern int wk_set_trajectory(IntPtr ctx, int horizon, float[] states, float[] actions, float[] logp, float[] rewards, byte[] dones, float[] values);
    [DllImport(Lib)] public static extern int wk_compute_returns(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_get_bootstrap_values(IntPtr ctx, float[] v);
    [DllImport(Lib)] public static extern int wk_set_bootstrap_values(IntPtr ctx, float[] v);
    [DllImport(Lib)] public static extern int wk_ppo_update(IntPtr ctx, ref WkPpoArgs args, out float criticDiag, out float actorDiag);
    [DllImport(Lib)] public static extern int wk_policy_stats(IntPtr ctx, out WkPpoStats stats, float[]? logpNew, float[]? valuesNew);
    [DllImport(Lib)] public static extern int wk_update_stats_get(IntPtr ctx, out WkPpoStats stats);
    [DllImport(Lib)] public static extern void wk_ppo_sums_add(ref WkPpoSums acc, ref WkPpoSums x);
    [DllImport(Lib)] public static extern void wk_ppo_stats_from_sums(ref WkPpoSums sums, out WkPpoStats stats);
    [DllImport(Lib)] public static extern void wk_log_std_grad_from_sums(ref WkPpoSums sums, float entropyCoef, out WkLogStdGrad grad);
    // global: IntPtr.Zero for this rank's record alone; else a WkPpoSums' address (collective on a record-exchange context)
    [DllImport(Lib)] public static extern int wk_policy_sums(IntPtr ctx, out WkPpoSums local, IntPtr globalOrNull);
    [DllImport(Lib)] public static extern int wk_policy_stats_global(IntPtr ctx, out WkPpoStats stats);
    [DllImport(Lib)] public static extern int wk_grad_norms_get(IntPtr ctx, out WkGradNorms norms);
    [DllImport(Lib)] public static extern int wk_set_learning_rate(IntPtr ctx, float alpha);
    [DllImport(Lib)] public static extern int wk_get_learning_rate(IntPtr ctx, out float alpha);
    [DllImport(Lib)] public static extern int wk_get_log_std(IntPtr ctx, out WkLogStdState state);
    [DllImport(Lib)] public static extern int wk_set_log_std(IntPtr ctx, float logStd);
    [DllImport(Lib)] public static extern int wk_set_log_std_adam(IntPtr ctx, double m, double v, int t);
    [DllImport(Lib)] public static extern int wk_log_std_gradient(IntPtr ctx, out WkLogStdGrad grad);
    [DllImport(Lib)] public static extern void wk_reward_norm_defaults(ref WkRewardNormArgs args);
    [DllImport(Lib)] public static extern int wk_reward_norm_config(IntPtr ctx, ref WkRewardNormArgs args);
    [DllImport(Lib)] public static extern int wk_reward_norm_get(IntPtr ctx, out WkRewardNorm state);
    [DllImport(Lib)] public static extern int wk_reward_norm_set(IntPtr ctx, long count, double mean, double m2);
    [DllImport(Lib)] public static extern int wk_reward_norm_get_acc(IntPtr ctx, [Out] float[] acc);
    [DllImport(Lib)] public static extern int wk_reward_norm_set_acc(IntPtr ctx, float[] acc);
    [DllImport(Lib)] public static extern int wk_reward_norm_update(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_get_scaled_rewards(IntPtr ctx, [Out] float[] rewards);
    [DllImport(Lib)] public static extern int wk_evaluate(IntPtr ctx, ref WkEvalArgs args, out WkEvalStats stats, [Out] WkEvalRec[]? recs);
    [DllImport(Lib)] public static extern int wk_evaluate_time(IntPtr ctx, int reps, out double stepMs, out double foldMs);
    [DllImport(Lib)] public static extern void wk_render_defaults(ref WkRenderArgs args);
    [DllImport(Lib)] public static extern int wk_render(IntPtr ctx, ref WkRenderArgs args, int[] envs, int nViews, [Out] byte[] rgba);
    [DllImport(Lib)] public static extern int wk_render_device(IntPtr ctx, ref WkRenderArgs args, int[] envs, int nViews, IntPtr deviceRgba);
    [DllImport(Lib)] public static extern int wk_render_states(IntPtr ctx, ref WkRenderArgs args, float[] states, int[] envs, int nViews, [Out] byte[] rgba);
    [DllImport(Lib)] public static extern int wk_train_batch(IntPtr ctx, int B, float bDiv, float[] states, float[] actions, float[] logpOld, float[] returns, float[] adv, out float criticDiag, out float actorDiag, float[]? gradsOut, int applyAdam, out int skipped);
    [DllImport(Lib)] public static extern int wk_minibatch_gradient(IntPtr ctx, int B, float bDiv, float[] states, float[] actions, float[] logpOld, float[] returns, float[] adv, out float criticDiag, out float actorDiag, float[]? gradsOut, out int skipped);

    // data collection (ConsoleRenderer.AddTotalEpisodeReward / AddCriticLoss / AddActorLoss / CreateDataFile)
    [DllImport(Lib)] public static extern int wk_collect_data(IntPtr ctx, int on);
    [DllImport(Lib)] public static extern int wk_episode_log_count(IntPtr ctx, out long episodes, out long updates);
    [DllImport(Lib)] public static extern int wk_episode_log_drain(IntPtr ctx, [Out] WkEpisodeRec[] recs, long cap, out long n, out long dropped);
    [DllImport(Lib)] public static extern int wk_loss_log_drain(IntPtr ctx, float[] critic, float[] actor, long cap, out long n, out long dropped);
    [DllImport(Lib, CharSet = CharSet.Ansi)] public static extern int wk_write_data_file(string path, float[] totalRewards, long nRewards, float[] criticLosses, long nCritic, float[] actorLosses, long nActor);

    // multi-GPU (one process per GPU)
    [DllImport(Lib)] public static extern int wk_comm_unique_id(byte[] id);
    [DllImport(Lib)] public static extern int wk_comm_init(IntPtr ctx, int rank, int nRanks, byte[] uniqueId);
    [DllImport(Lib)] public static extern int wk_allreduce_test(IntPtr ctx, float[] buf, int n);
    [DllImport(Lib)] public static extern int wk_comm_ipc_handle(IntPtr ctx, byte[] handle);
    [DllImport(Lib)] public static extern int wk_comm_init_ipc(IntPtr ctx, int rank, int nRanks, byte[] handles);
    [DllImport(Lib)] public static extern int wk_comm_info(IntPtr ctx, out int kind, out int flags);
    [DllImport(Lib)] public static extern int wk_comm_set_timeout(IntPtr ctx, double seconds);
    [DllImport(Lib)] public static extern int wk_comm_xch_profile(IntPtr ctx, int minibatches);
    [DllImport(Lib)] public static extern int wk_comm_xch_stamps(IntPtr ctx, ulong[] stamps, int maxLaunches, out int launches, out int blocks);
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)] public delegate int HostAllReduce(IntPtr buf, int n, IntPtr user);
    [DllImport(Lib)] public static extern int wk_comm_init_host(IntPtr ctx, int rank, int nRanks, HostAllReduce fn, IntPtr user);

    // The record exchange (before wk_comm_init / wk_comm_init_host): fn is IntPtr.Zero for RCCL, else the function pointer
    // of a HostAllGather (mine: 16 words in, all: nRanks * 16 words out, rank order).  Use CommRecords, which keeps the
    // delegate reachable for the context's lifetime as CommInitHost does.
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)] public delegate int HostAllGather(IntPtr mine, IntPtr all, IntPtr user);
    [DllImport(Lib)] public static extern int wk_comm_records(IntPtr ctx, IntPtr fnOrNull, IntPtr user);
    static readonly System.Collections.Concurrent.ConcurrentDictionary<IntPtr, HostAllGather> s_hostAllGather = new();
    public static int CommRecords(IntPtr ctx, HostAllGather? fn, IntPtr user)
    {
        int rc = wk_comm_records(ctx, fn == null ? IntPtr.Zero : Marshal.GetFunctionPointerForDelegate(fn), user);
        if (rc == 0 && fn != null) s_hostAllGather[ctx] = fn;
        return rc;
    }

    // libwk keeps the function pointer for the context's lifetime; the marshalled thunk dies with
    // the delegate, so the delegate must stay reachable until the context is destroyed.  Use
    // CommInitHost / Destroy instead of the raw entry points when a host all-reduce is set.
    // A failing callback (non-zero return) fails that rank's wk_ppo_update with WK_ERR_COMM
    // while its peers wait in their own all-reduce: treat it as fatal for the whole job.
    static readonly System.Collections.Concurrent.ConcurrentDictionary<IntPtr, HostAllReduce> s_hostAllReduce = new();
    public static int CommInitHost(IntPtr ctx, int rank, int nRanks, HostAllReduce fn, IntPtr user)
    {
        int rc = wk_comm_init_host(ctx, rank, nRanks, fn, user);
        if (rc == 0) s_hostAllReduce[ctx] = fn;
        return rc;
    }
    public static int Destroy(IntPtr ctx)
    {
        int rc = wk_destroy(ctx);
        s_hostAllReduce.TryRemove(ctx, out _);
        s_hostAllGather.TryRemove(ctx, out _);
        return rc;
    }

    // profiling, counting replay, snapshots
    [DllImport(Lib)] public static extern int wk_profile_enable(IntPtr ctx, int on);
    [DllImport(Lib)] public static extern int wk_profile_get(IntPtr ctx, out WkProfile profile);
    [DllImport(Lib)] public static extern int wk_profile_reset(IntPtr ctx);
    [DllImport(Lib)] public static extern int wk_count_events(IntPtr ctx, int k, ulong[] counts);
    [DllImport(Lib)] public static extern int wk_snapshot(IntPtr ctx, int op);
    [DllImport(Lib)] public static extern int wk_time_gradient(IntPtr ctx, int minibatch, int reps, out double msPerLaunch);
    [DllImport(Lib)] public static extern int wk_time_gradient_ex(IntPtr ctx, int minibatch, int reps, int flags, out double msPerLaunch);
    [DllImport(Lib)] public static extern int wk_rollout_mapping(IntPtr ctx, out int lanesPerWalker, out int walkersPerWave, out long waves, out long wavesLaunched);
    [DllImport(Lib)] public static extern int wk_grad_kernel(IntPtr ctx, int minibatch);

    public static string LastError(IntPtr ctx) => Marshal.PtrToStringAnsi(wk_last_error(ctx)) ?? "";

    // log-and-continue, like every try/catch -> ErrorLogger.LogError in the reference
    public static bool Ok(IntPtr ctx, int rc, string what, Action<string>? log = null)
    {
        if (rc == 0) return true;
        (log ?? Console.Error.WriteLine)($"{what}: {LastError(ctx)} ({(WkStatus)rc})");
        return false;
    }
}
