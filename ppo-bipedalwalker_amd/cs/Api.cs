// Api.cs -- the reference's object API (IMaterial, IObject, RigidBody, Walker) over libwk.so, so a
// C# host that used NEA.Materials / NEA.Objects / NEA.Walker keeps compiling against the same
// names: Materials/IMaterial.cs:6-12 and the eight materials, Objects/IObject.cs:7-10,
// Bodies/RigidBody.cs (the read side a renderer and GetState use), Walker/Walker.cs:49-223.
// The C++ mirror of the same surface is csrc/host/nea.hpp; this file follows it member for
// member.  The physics state lives on the GPU (one context per environment), so a RigidBody
// here is a view of one body of one walker (wk_get_body_view).  A host that keeps the reference's
// Environment.StepObjects loop (Environment.cs:126-143: per substep Joint.Step on the 4 joints,
// then IObject.Update on every body of the list) calls wk_object_update list.Count * Iterations
// times per frame: the frame's first call runs the env-step of every walker with the torques
// Walker.TakeActions stored (wk_take_actions), the others are counted no-ops.  Errors are logged
// and the operation skipped (ErrorLogger.LogError, the reference's convention).
using System;
using System.Collections.Generic;

namespace NEA.Materials
{
    // Materials/IMaterial.cs:6-12 (Color omitted: headless); Id selects the kernel's table
    public interface IMaterial
    {
        float InverseMass { get; }
        float Friction { get; }
        float Restitution { get; }
        int Id { get; }
    }
    // Materials/<Name>.cs: the constants of csrc/wk_common.h material() and nea.hpp
    public sealed class Carpet : IMaterial { public float InverseMass => 5f; public float Friction => 0.8f; public float Restitution => 0.3f; public int Id => 0; }
    public sealed class Ice : IMaterial { public float InverseMass => 11f; public float Friction => 0f; public float Restitution => 0.3f; public int Id => 1; }
    public sealed class Rubber : IMaterial { public float InverseMass => 11f; public float Friction => 0.5f; public float Restitution => 0.7f; public int Id => 2; }
    public sealed class Metal : IMaterial { public float InverseMass => 15f; public float Friction => 1f; public float Restitution => 0.3f; public int Id => 3; }
    public sealed class Wood : IMaterial { public float InverseMass => 20f; public float Friction => 0.01f; public float Restitution => 0.3f; public int Id => 4; }
    public sealed class Paper : IMaterial { public float InverseMass => 1f; public float Friction => 0.1f; public float Restitution => 0.3f; public int Id => 5; }
    public sealed class Titanium : IMaterial { public float InverseMass => 0.01f; public float Friction => 0.2f; public float Restitution => 0.1f; public int Id => 6; }
    public sealed class SuperRubber : IMaterial { public float InverseMass => 11f; public float Friction => 1f; public float Restitution => 1f; public int Id => 7; }
}

namespace NEA.Objects
{
    using NEA.Bodies;

    // Objects/IObject.cs:7-10
    public interface IObject
    {
        void Update(List<RigidBody> rigidBodies, float deltaTime);
    }
}

namespace NEA.Bodies
{
    using NEA.Native;
    using NEA.Objects;

    // Bodies/RigidBody.cs, the read side (GetVertices / GetCentroid / GetLinearVelocity /
    // GetAngularVelocity / GetAngle / Collided / IsStatic) of body `Part` (0 LLL, 1 LLU, 2 Body,
    // 3 RLL, 4 RLU, 5 Floor -- 5..14 the rough floor's segments) of walker `Env`.
    // Update (IObject): the GPU resolves every body of the list in the reference's order inside
    // one env-step, so stepping one body alone does not exist; the frame is assembled natively.
    public sealed class RigidBody : IObject
    {
        readonly IntPtr _ctx;
        public int Env { get; }
        public int Part { get; }
        internal RigidBody(IntPtr ctx, int env, int part) { _ctx = ctx; Env = env; Part = part; }

        WkBodyView View()
        {
            Wk.Ok(_ctx, Wk.wk_get_body_view(_ctx, Env, Part, out var v), "Exception while reading a rigid body", Console.Error.WriteLine);
            return v;
        }
        public unsafe List<(float X, float Y)> GetVertices()
        {
            var v = View();
            var l = new List<(float, float)>(v.NVertices);
            for (int i = 0; i < v.NVertices; i++) l.Add((v.Vertices[2 * i], v.Vertices[2 * i + 1]));
            return l;
        }
        public unsafe (float X, float Y) GetCentroid() { var v = View(); return (v.Centroid[0], v.Centroid[1]); }
        public unsafe (float X, float Y) GetLinearVelocity() { var v = View(); return (v.LinearVelocity[0], v.LinearVelocity[1]); }
        public float GetAngularVelocity() => View().AngularVelocity;
        public float GetAngle() => View().Angle;
        public bool Collided => View().Collided != 0;
        public bool IsStatic => View().IsStatic != 0;

        // IObject.Update (Objects/IObject.cs:9), called list.Count * Iterations times per frame by
        // Environment.StepObjects (Environment.cs:130-141): the frame's first call steps every
        // walker of the context once with the torques Walker.TakeActions stored (a walker given
        // none keeps its torques: no kick), the frame's other calls are no-ops (wk_object_update)
        public void Update(List<RigidBody> rigidBodies, float deltaTime)
        {
            int r = Wk.wk_object_update(_ctx, rigidBodies.Count, deltaTime);
            if (r < 0) Wk.Ok(_ctx, r, "Exception occurred during the environment update", Console.Error.WriteLine);
        }
    }

    // Joint.Step (Joint.cs:31-41): the joints of every walker are resolved inside the frame's
    // env-step (wk_joint_step is a no-op kept for the call shape)
    public sealed class Joint
    {
        readonly IntPtr _ctx;
        internal Joint(IntPtr ctx) { _ctx = ctx; }
        public void Step() => Wk.wk_joint_step(_ctx);
    }
}

namespace NEA.Walker
{
    using NEA.Bodies;
    using NEA.Materials;
    using NEA.Native;
    using NEA.Objects;

    // What an update did to the policy (no counterpart in the reference, which reports two loss
    // numbers): the current networks on the context's trajectory buffer -- approximate KL to the
    // collecting policy, clip fraction, explained variance -- and the last per-epoch check of a
    // TargetKL > 0 update.  null on failure, logged like every other call
    public static class PolicyStatistics
    {
        public static WkPpoStats? Current(IntPtr ctx, float[]? logpNew = null, float[]? valuesNew = null, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_policy_stats(ctx, out var s, logpNew, valuesNew), "Exception while reading the policy statistics", log) ? s : null;

        public static WkPpoStats? LastUpdate(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_update_stats_get(ctx, out var s), "Exception while reading the update's statistics", log) ? s : null;

        // over all the ranks' shards: collective on a record-exchange context (RecordExchange.Declare)
        public static WkPpoStats? Global(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_policy_stats_global(ctx, out var s), "Exception while reading the global policy statistics", log) ? s : null;

        // this rank's raw sums, as the record exchange gathers them
        public static WkPpoSums? Sums(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_policy_sums(ctx, out var s, IntPtr.Zero), "Exception while reading the policy sums", log) ? s : null;

        public static WkPpoSums Add(WkPpoSums acc, WkPpoSums x) { Wk.wk_ppo_sums_add(ref acc, ref x); return acc; }
        public static WkPpoStats FromSums(WkPpoSums sums) { Wk.wk_ppo_stats_from_sums(ref sums, out var s); return s; }
        public static WkLogStdGrad LogStdGradFromSums(WkPpoSums sums, float entropyCoef) { Wk.wk_log_std_grad_from_sums(ref sums, entropyCoef, out var g); return g; }
    }

    // TargetKL, LearnLogStd and reward normalisation on several GPUs: declared before the gradient
    // exchange is initialised, the ranks then gather their statistics records and every rank decides
    // on the same fold.  gather null: RCCL (then wk_comm_init); else the host control plane (then
    // Wk.CommInitHost)
    public static class RecordExchange
    {
        public static bool Declare(IntPtr ctx, Wk.HostAllGather? gather = null, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.CommRecords(ctx, gather, IntPtr.Zero), "Exception while declaring the record exchange", log);
    }

    // The size of the optimiser's steps (no counterpart in the reference): the per-network gradient
    // norms of the last update's Adam steps on a MaxGradNorm > 0 context, and the learning rate a
    // host may anneal between updates (Alpha is otherwise fixed at wk_create).  null / false on
    // failure, logged like every other call
    public static class Optimiser
    {
        public static WkGradNorms? GradNorms(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_grad_norms_get(ctx, out var g), "Exception while reading the gradient norms", log) ? g : null;

        public static bool SetLearningRate(IntPtr ctx, float alpha, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_set_learning_rate(ctx, alpha), "Exception while setting the learning rate", log);

        public static float? LearningRate(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_get_learning_rate(ctx, out var a), "Exception while reading the learning rate", log) ? a : null;
    }

    // The policy's exploration noise (LogStandardDeviation is a constant in the reference): the
    // scalar log-std a LearnLogStd = 1 context trains after every epoch, or a host anneals itself
    // with Set on any context; Gradient is the pass alone.  null / false on failure, logged
    public static class LogStd
    {
        public static WkLogStdState? State(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_get_log_std(ctx, out var s), "Exception while reading the log standard deviation", log) ? s : null;

        public static bool Set(IntPtr ctx, float logStd, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_set_log_std(ctx, logStd), "Exception while setting the log standard deviation", log);

        public static bool SetAdam(IntPtr ctx, double m, double v, int t, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_set_log_std_adam(ctx, m, v, t), "Exception while setting the log standard deviation's Adam state", log);

        public static WkLogStdGrad? Gradient(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_log_std_gradient(ctx, out var g), "Exception while reading the log standard deviation's gradient", log) ? g : null;
    }

    // Reward normalisation (the reference trains on the raw rewards, Environment.cs:148-154): the
    // rewards the returns read are scaled by the running std of the walkers' discounted returns;
    // the trajectory's own rewards, the episode log and the evaluation stay raw.  Switched on per
    // context at run time.  null / false on failure, logged
    public static class RewardNorm
    {
        public static bool Configure(IntPtr ctx, bool enable = true, float clip = 10.0f, float epsilon = 1e-8f, bool frozen = false,
                                     Action<string>? log = null)
        {
            var a = new WkRewardNormArgs();
            Wk.wk_reward_norm_defaults(ref a);
            a.Enable = enable ? 1 : 0; a.Frozen = frozen ? 1 : 0; a.Clip = clip; a.Epsilon = epsilon;
            return Wk.Ok(ctx, Wk.wk_reward_norm_config(ctx, ref a), "Exception while configuring the reward normalisation", log);
        }

        public static WkRewardNorm? State(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_reward_norm_get(ctx, out var s), "Exception while reading the reward normalisation", log) ? s : null;

        public static bool SetState(IntPtr ctx, long count, double mean, double m2, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_reward_norm_set(ctx, count, mean, m2), "Exception while setting the reward statistics", log);

        public static float[]? Acc(IntPtr ctx, Action<string>? log = null)
        {
            var a = new float[Wk.wk_num_envs(ctx)];
            return Wk.Ok(ctx, Wk.wk_reward_norm_get_acc(ctx, a), "Exception while reading the running returns", log) ? a : null;
        }

        public static bool SetAcc(IntPtr ctx, float[] acc, Action<string>? log = null) =>
            acc.Length == Wk.wk_num_envs(ctx) &&
            Wk.Ok(ctx, Wk.wk_reward_norm_set_acc(ctx, acc), "Exception while setting the running returns", log);

        // the full pass on the current trajectory buffer (after wk_set_trajectory, whose data is scaled but not learned)
        public static bool Update(IntPtr ctx, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_reward_norm_update(ctx), "Exception while updating the reward statistics", log);

        // the [horizon][n] rewards the returns kernels read; horizon = the rows of the trajectory buffer
        public static float[]? ScaledRewards(IntPtr ctx, int horizon, Action<string>? log = null)
        {
            var r = new float[(long)horizon * Wk.wk_num_envs(ctx)];
            return Wk.Ok(ctx, Wk.wk_get_scaled_rewards(ctx, r), "Exception while reading the scaled rewards", log) ? r : null;
        }
    }

    // How good the policy is now (the counterpart of the console's _bestDistance and last-episode
    // average reward, Environment.cs:55-60,119): every walker plays complete episodes under the
    // current actor -- its mean action unless args.Stochastic -- on a private copy of the walker
    // state, so a call between two updates changes nothing of the run.  records (optional) holds
    // Episodes * wk_num_envs slots, layout [episode][walker].  null on failure, logged
    public static class Evaluation
    {
        public static WkEvalStats? Run(IntPtr ctx, WkEvalArgs args = default, WkEvalRec[]? records = null, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_evaluate(ctx, ref args, out var s, records), "Exception while evaluating the policy", log) ? s : null;

        // mean milliseconds per launch of the accounting kernel and of the fold, on the last Run's block
        public static (double StepMs, double FoldMs)? KernelTimes(IntPtr ctx, int reps = 64, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_evaluate_time(ctx, reps, out var st, out var fo), "Exception while timing the evaluation kernels", log) ? (st, fo) : null;
    }

    // Frames (the counterpart of Environment.RenderObjects, Environment.cs:189-208): the listed
    // walkers drawn on the device into RGBA bytes [view][row][column][4], row 0 at the top.  Render
    // draws the context's records as they are, RenderStates host records in wk_get_state's layout
    // (a saved episode) with the listed walkers' materials, terrain and props.  null on failure, logged
    public static class Frames
    {
        public static WkRenderArgs Defaults()
        {
            var a = new WkRenderArgs();
            Wk.wk_render_defaults(ref a);
            return a;
        }

        public static byte[]? Render(IntPtr ctx, WkRenderArgs args, int[] envs, Action<string>? log = null)
        {
            var img = new byte[(long)envs.Length * args.Height * args.Width * 4];
            return Wk.Ok(ctx, Wk.wk_render(ctx, ref args, envs, envs.Length, img), "Exception while rendering", log) ? img : null;
        }

        public static byte[]? RenderStates(IntPtr ctx, WkRenderArgs args, float[] states, int[] envs, Action<string>? log = null)
        {
            var img = new byte[(long)envs.Length * args.Height * args.Width * 4];
            return Wk.Ok(ctx, Wk.wk_render_states(ctx, ref args, states, envs, envs.Length, img), "Exception while rendering saved states", log) ? img : null;
        }

        // the same frames into device memory (4-byte aligned) on the context's stream: no copy, no synchronise
        public static bool RenderDevice(IntPtr ctx, WkRenderArgs args, int[] envs, IntPtr deviceRgba, Action<string>? log = null) =>
            Wk.Ok(ctx, Wk.wk_render_device(ctx, ref args, envs, envs.Length, deviceRgba), "Exception while rendering to device memory", log);
    }

    // Walker/Walker.cs:49-223 for walker `Index` of a context (a Walker owns no state of its own:
    // its bodies, torques, Collided flags and episode counter live in the context's records)
    public sealed class Walker
    {
        readonly IntPtr _ctx;
        readonly Action<string> _log;
        public int Index { get; }
        public IMaterial Material { get; }

        public Walker(IntPtr ctx, int index, IMaterial? material = null, Action<string>? log = null)
        {
            _ctx = ctx;
            Index = index;
            _log = log ?? Console.Error.WriteLine;
            Material = material ?? new Carpet();  // Walker.cs:28 (_material = new Carpet())
        }

        // CreateCreature (Walker.cs:38-44): the context created every walker's bodies, joints,
        // associated bodies and gravity at wk_create (the materials: wk_set_materials, from the
        // host's IMaterial.Id per walker); this fills the caller's list with the walker's bodies
        public void CreateCreature(List<RigidBody> rigidBodies)
        {
            rigidBodies.Clear();
            rigidBodies.AddRange(Bodies());
        }

        // the list RigidBody.ResolveCollisions walks, in its current order (wk_body_order):
        // [LLL, LLU, Body, RLL, RLU, Floor] in episode 0, [Floor, LLL, LLU, Body, RLL, RLU] after a
        // reset (Reset removes the walker's bodies and CreateBodies appends them after the floor,
        // Walker.cs:191-234); the rough floor's ten segments stand where the floor does
        public List<RigidBody> Bodies()
        {
            var parts = new int[15];
            var l = new List<RigidBody>(15);
            if (!Wk.Ok(_ctx, Wk.wk_body_order(_ctx, Index, parts, out int n), "Exception while reading the body list", _log))
                return l;
            for (int i = 0; i < n; i++) l.Add(new RigidBody(_ctx, Index, parts[i]));
            return l;
        }

        // the part of this walker's list (by part id, whatever the list order)
        RigidBody Part(int part) => new RigidBody(_ctx, Index, part);

        // GetJoints (Walker.cs:102): [bodyJointLeft, bodyJointRight, leftJoint, rightJoint]
        public List<Joint> GetJoints() => new List<Joint> { new(_ctx), new(_ctx), new(_ctx), new(_ctx) };

        // Walker.Update (:49-54): terminal once the body or an upper leg touched the floor
        public bool Terminal => Part(2).Collided || Part(1).Collided || Part(4).Collided;

        // GetActions (:57-62): the policy's sample for this walker's state
        public float[] GetActions(float[] state, out float[] logProbabilities)
        {
            var a = new float[WkConst.Act];
            var mean = new float[WkConst.Act];
            logProbabilities = new float[WkConst.Act];
            var ids = new[] { Index };
            Wk.Ok(_ctx, Wk.wk_policy_sample(_ctx, 1, state, ids, null, mean, a, logProbabilities),
                  "Exception thrown while attempting to sample actions", _log);
            return a;
        }

        // TakeActions (:66-75): the torques of the next frame; a wrong-sized action is ignored
        // like the reference's height check; the joints' SetTorque runs inside the step
        public void TakeActions(float[] actions)
        {
            if (actions.Length != WkConst.Act) return;
            Wk.Ok(_ctx, Wk.wk_take_actions(_ctx, Index, actions), "Exception while setting the torques", _log);
        }

        // GetState (:132-152)
        public float[] GetState()
        {
            int n = Wk.wk_num_envs(_ctx);
            var all = new float[n * WkConst.Obs];
            var s = new float[WkConst.Obs];
            if (Wk.Ok(_ctx, Wk.wk_get_obs(_ctx, all), "Exception while reading the walker state", _log))
                Array.Copy(all, Index * WkConst.Obs, s, 0, WkConst.Obs);
            return s;
        }

        // GetPosition (:108-111): the torso's centroid
        public (float X, float Y) GetPosition() => Part(2).GetCentroid();

        // Reset (:212-223): this walker back to its template (post-reset list order)
        public void Reset(List<RigidBody> rigidBodies)
        {
            var mask = new byte[Wk.wk_num_envs(_ctx)];
            mask[Index] = 1;
            Wk.Ok(_ctx, Wk.wk_reset(_ctx, mask), "Exception while resetting the walker", _log);
            rigidBodies.Clear();
            rigidBodies.AddRange(Bodies());
        }
    }
}
