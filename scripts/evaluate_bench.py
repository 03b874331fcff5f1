"""What an evaluation costs (wk_evaluate), one GPU, 65,536 walkers, default network strings,
RandomizeStart.  A warm-up, then `--calls` calls per figure, timed with the host clock around the
synchronous call; every figure is recorded with its spread.

  1. evaluate(episodes=1) -- wall time and time per env-step (wall / steps_run) -- on a built-in
     context and on a NetworkKernels = 1 context.
  2. beside it the per-env-step time of a NetworkKernels = 1 rollout on the same build (the figure
     of scripts/net_bench.py: rollout(T_h) / T_h, host clock around rollout + sync): the same three
     launches per env-step without the accounting kernel.
  3. in a run of their own, the accounting kernel's and the fold's durations from HIP events
     (wk_evaluate_time: a burst of back-to-back launches between one event pair), and the
     accounting kernel's share of the evaluation's env-step.

  python scripts/evaluate_bench.py [--walkers N] [--calls 5] [--reps 64] [--out profiles/evaluate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-bipedalwalker_amd"))
import wk  # noqa: E402

STEP_BYTES = 4 + 1 + 4 + 2 * (8 + 4 + 4) + 4  # reward, done, x; sum, length, best x both ways; episode index


def spread(v, unit="ms"):
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v),
            f"stdev_{unit}": statistics.pstdev(v), "calls": len(v)}


def engine(args, kernels):
    return wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, RandomizeStart=1, NetworkKernels=kernels)


def time_evaluate(args, kernels):
    eng = engine(args, kernels)
    eng.evaluate(max_steps=64)  # warm: every kernel of the loop, the private block
    wall, per_step, st = [], [], None
    for _ in range(args.calls):
        t0 = time.perf_counter()
        st = eng.evaluate(episodes=1)
        ms = (time.perf_counter() - t0) * 1e3
        wall.append(ms)
        per_step.append(ms / st["steps_run"])
    out = {"wall": spread(wall), "per_env_step": spread(per_step),
           "mapping": eng.rollout_mapping()["lanes_per_walker"],
           "stats": {k: st[k] for k in ("episodes", "fell", "timed_out", "succeeded", "steps_run", "env_steps",
                                        "reward_mean", "reward_std", "length_mean", "distance_mean", "distance_max")}}
    out["walker_steps_per_s"] = st["env_steps"] / (out["wall"]["median_ms"] * 1e-3)
    eng.close()
    return out


def time_rollout(args):
    eng = engine(args, 1)
    eng.collect_data(False)
    eng.rollout(args.horizon)
    eng.sync()
    ms = []
    for _ in range(max(args.calls, 5)):
        t0 = time.perf_counter()
        eng.rollout(args.horizon)
        eng.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / args.horizon)
    eng.close()
    return {"per_env_step": spread(ms), "horizon": args.horizon}


def time_kernels(args):
    eng = engine(args, 0)
    step, fold = [], []
    for _ in range(max(args.calls, 5)):
        eng.evaluate(max_steps=8)
        s, f = eng.evaluate_time(args.reps)
        step.append(s * 1e3)
        fold.append(f * 1e3)
    eng.close()
    out = {"accounting_kernel": spread(step, "us"), "fold_kernels": spread(fold, "us"), "burst": args.reps,
           "accounting_bytes_per_walker_step": STEP_BYTES}
    out["accounting_tb_per_s"] = STEP_BYTES * args.walkers / (out["accounting_kernel"]["median_us"] * 1e-6) / 1e12
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=65536)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--reps", type=int, default=64)
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate.json"))
    args = p.parse_args()
    res = {"shape": {"walkers": args.walkers, "networks": "default strings", "RandomizeStart": 1},
           "clock": "host clock around synchronous calls; kernels: HIP events around a burst"}
    for name, kernels in (("builtin", 0), ("general_default", 1)):
        res[f"evaluate_{name}"] = time_evaluate(args, kernels)
        print(json.dumps({f"evaluate_{name}": res[f"evaluate_{name}"]}), flush=True)
    res["rollout_general_default"] = time_rollout(args)
    print(json.dumps({"rollout_general_default": res["rollout_general_default"]}), flush=True)
    res["kernels"] = time_kernels(args)
    step_ms = res["evaluate_general_default"]["per_env_step"]["median_ms"]
    res["evaluate_over_rollout_per_env_step"] = step_ms / res["rollout_general_default"]["per_env_step"]["median_ms"]
    res["accounting_share_of_env_step"] = res["kernels"]["accounting_kernel"]["median_us"] * 1e-3 / step_ms
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
