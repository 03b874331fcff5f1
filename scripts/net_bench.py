"""What generality costs: the general networks' kernels (NetworkKernels = 1) against the built-in
ones (NetworkKernels = 0) on the default network strings, same build, one GPU, at bench.py's
shape (65,536 walkers, T_h 64, M 65,536, 5 epochs; the snapshot restored before every timed
iteration, as bench.py does) -- rollout ms and update ms, and one iteration's per-launch profile
(level 2: gradient / reduction+Adam launches).  Then, for the widest network of the test list
(tests/netref.py `max`, 70,021 parameters), the gradient kernel's ms per launch through
wk_time_gradient and its TFLOP/s, counted as 6 * sum(out * in) flop per sample (forward, input
gradient and weight gradient of every dense layer, 2 flop per multiply-add) against the
157.3 TFLOP/s fp32 matrix-core peak.

  python scripts/net_bench.py [--walkers N] [--horizon T] [--minibatch M] [--epochs E]
                              [--steps K] [--regime-iters R] [--out profiles/net_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ppo-bipedalwalker_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import wk  # noqa: E402
import netref  # noqa: E402

PEAK_TFLOPS = 157.3


def flop_per_sample(critic, actor):
    return 6 * sum(i * o for dsl in (critic, actor) for k, i, o in netref.layers(dsl) if k == "D")


def time_path(args, kernels):
    eng = wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                    Epochs=args.epochs, RandomizeStart=1, NetworkKernels=kernels)
    for it in range(args.regime_iters):
        eng.rollout(args.horizon)
        eng.ppo_update(update_index=it, sync=False)
    eng.snapshot()

    def iterations(k):
        for j in range(k):
            eng.restore()
            eng.rollout(args.horizon)
            eng.ppo_update(update_index=args.regime_iters + j, sync=False)
        eng.sync()

    iterations(1)
    eng.profile_reset()
    eng.profile_enable(1)
    iterations(args.steps)
    prof = eng.profile()
    eng.profile_reset()
    eng.profile_enable(2)
    iterations(1)
    p2 = eng.profile()
    eng.profile_enable(0)
    out = {
        "grad_kernel": eng.grad_kernel(),
        "rollout_ms": prof["physics_ms"] / max(1, prof["physics_launches"]),
        "update_ms": prof["update_ms"] / max(1, prof["update_calls"]),
        "minibatches_per_update": p2["grad_launches"],
        "level2_grad_ms_per_launch": p2["grad_ms"] / max(1, p2["grad_launches"]),
        "level2_reduce_adam_ms_per_launch": (p2["reduce_ms"] + p2["adam_ms"]) / max(1, p2["reduce_launches"]),
        "level2_update_ms": p2["update_ms"],
        "grad_burst_ms_per_launch": eng.time_gradient(args.minibatch, args.burst),
    }
    eng.close()
    return out


def time_widest(args):
    c, a = netref.NETS["max"]
    eng = wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                    RandomizeStart=1, NetworkKernels=1, CriticNeuralNetwork=c, ActorNeuralNetwork=a)
    eng.rollout(args.horizon)
    ms = eng.time_gradient(args.minibatch, args.burst)
    flop = flop_per_sample(c, a) * args.minibatch
    out = {"critic": c, "actor": a, "parameters": eng.nparam, "minibatch": args.minibatch,
           "flop_per_sample": flop_per_sample(c, a), "grad_ms_per_launch": ms,
           "tflops": flop / (ms * 1e-3) / 1e12,
           "fraction_of_fp32_mfma_peak": flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS}
    eng.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=65536)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--minibatch", type=int, default=65536)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--steps", type=int, default=2)
    p.add_argument("--regime-iters", type=int, default=2)
    p.add_argument("--burst", type=int, default=4)
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_bench.json"))
    args = p.parse_args()
    res = {"shape": {"walkers": args.walkers, "horizon": args.horizon, "minibatch": args.minibatch,
                     "epochs": args.epochs, "timed_iterations": args.steps,
                     "regime_iterations": args.regime_iters},
           "builtin_default": time_path(args, 0)}
    print(json.dumps({"builtin_default": res["builtin_default"]}), flush=True)
    res["general_default"] = time_path(args, 1)
    print(json.dumps({"general_default": res["general_default"]}), flush=True)
    b, g = res["builtin_default"], res["general_default"]
    res["general_over_builtin"] = {"rollout": g["rollout_ms"] / b["rollout_ms"],
                                   "update": g["update_ms"] / b["update_ms"]}
    res["general_widest"] = time_widest(args)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
