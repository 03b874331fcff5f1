"""What the trained log-std costs (LearnLogStd, the pass of wk_log_std_gradient after every epoch),
one GPU, at bench.py's shape (65,536 walkers, T_h 64: 4.19 M rows; M 65,536: 5 epochs of 64
minibatches).  A warm-up, then at least 20 updates per figure, each from its context's snapshot,
timed with the host clock around synchronised calls; the arms alternate A B A B and every figure is
recorded with its spread (median, min, max).

  1. wk_ppo_update with LearnLogStd 0 against 1, and with TargetKL = 1e9 (a check after every
     epoch, never a stop) against TargetKL = 1e9 and LearnLogStd = 1: the claim to check is one
     pass per epoch, not two.
  2. wk_log_std_gradient and wk_policy_stats per call (the two instantiations of the pass).
  3. with --parent-root DIR (a built checkout of the parent commit): the LearnLogStd = 0 update of
     this tree against the parent's, alternated, every run a fresh process, and `python bench.py`'s
     headline of the two trees, alternated; the margin is the spread of the parent's own runs.
  4. a training trace: 4,096 walkers, LearnLogStd = 1, LogStdAlpha = 1e-2, EntropyCoef = 0, 20
     iterations of rollout + update, printing log_std, z2_mean and the evaluation's mean reward.
     Recorded, nothing asserted.

  python scripts/log_std_bench.py [--calls 20] [--runs 5] [--bench-runs 3] [--parent-root DIR]
                                  [--out profiles/log_std.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.pstdev(ms), "calls": len(ms)}


def load(root):
    sys.path.insert(0, os.path.join(root, "ppo-bipedalwalker_amd"))
    import wk
    return wk


def engine(wk, args, **cfg):
    return wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                     Epochs=args.epochs, RandomizeStart=1, **cfg)


def prepare(e, args):
    e.rollout(args.horizon)
    e.snapshot()
    e.ppo_update(update_index=0, sync=False)  # warm
    e.sync()


def timed_update(e):
    e.restore()
    e.sync()
    t0 = time.perf_counter()
    e.ppo_update(update_index=0, sync=False)
    e.sync()
    return (time.perf_counter() - t0) * 1e3


def time_arms(wk, args):
    arms = {"off": {}, "learn": {"LearnLogStd": 1}, "kl": {"TargetKL": 1e9},
            "kl_learn": {"TargetKL": 1e9, "LearnLogStd": 1}}
    engs = {k: engine(wk, args, **cfg) for k, cfg in arms.items()}
    for e in engs.values():
        prepare(e, args)
    ms = {k: [] for k in engs}
    for _ in range(args.calls):
        for k, e in engs.items():
            ms[k].append(timed_update(e))
    out = {k: spread(v) for k, v in ms.items()}
    med = {k: out[k]["median_ms"] for k in out}
    out["ms_per_epoch_learn_minus_off"] = (med["learn"] - med["off"]) / args.epochs
    out["ms_per_epoch_kl_minus_off"] = (med["kl"] - med["off"]) / args.epochs
    out["ms_per_epoch_kl_learn_minus_kl"] = (med["kl_learn"] - med["kl"]) / args.epochs
    out["log_std_after_learn"] = engs["learn"].log_std()
    out["update_stats_kl_learn"] = engs["kl_learn"].update_stats()
    # the pass alone, both instantiations, on the context the update has moved
    e = engs["learn"]
    for name, call in (("log_std_gradient", e.log_std_gradient), ("policy_stats", e.policy_stats)):
        for _ in range(3):
            call()
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        out[f"{name}_call"] = spread(t)
    for e in engs.values():
        e.close()
    return out


def worker(args):
    """one fresh process: the median of --calls LearnLogStd = 0 updates of the tree at --tree"""
    wk = load(args.tree)
    e = engine(wk, args)
    prepare(e, args)
    ms = [timed_update(e) for _ in range(args.calls)]
    e.close()
    print(json.dumps(spread(ms)))


def against_parent(out, unit):
    out[f"parent_spread_{unit}"] = out["parent"]["max"] - out["parent"]["min"]
    out[f"this_minus_parent_{unit}"] = out["this"]["median"] - out["parent"]["median"]
    out["within_parent_spread"] = abs(out[f"this_minus_parent_{unit}"]) <= out[f"parent_spread_{unit}"]
    return out


def time_parent_update(args, trees):
    runs = {k: [] for k in trees}
    for _ in range(args.runs):
        for k, root in trees.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", root,
                                "--calls", str(args.calls), "--walkers", str(args.walkers),
                                "--horizon", str(args.horizon), "--minibatch", str(args.minibatch),
                                "--epochs", str(args.epochs), "--seed", str(args.seed)],
                               capture_output=True, text=True, timeout=600, check=True)
            runs[k].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["median_ms"])
            print(json.dumps({k: runs[k][-1]}), flush=True)
    out = {"what": "wk_ppo_update, LearnLogStd = 0 (this tree) against the parent commit; every run a fresh "
                   "process, its figure the median of --calls updates from the snapshot", "runs": args.runs}
    for k, v in runs.items():
        out[k] = {"median_ms_per_run": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    return against_parent(out, "ms")


def time_parent_bench(args, trees):
    runs = {k: [] for k in trees}
    for _ in range(args.bench_runs):
        for k, root in trees.items():
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps",
                                str(args.bench_steps), "--warmup", str(args.bench_warmup)], cwd=root,
                               capture_output=True, text=True, timeout=900, check=True)
            d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            runs[k].append(d["value"])
            print(json.dumps({k: d["value"]}), flush=True)
    out = {"command": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}",
           "unit": "env-steps/s", "runs": args.bench_runs}
    for k, v in runs.items():
        out[k] = {"per_run": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    out["this_over_parent"] = out["this"]["median"] / out["parent"]["median"]
    return against_parent(out, "env_steps_per_s")


def training_trace(wk, args):
    e = wk.Engine(4096, seed=args.seed, Horizon=args.horizon, Minibatch=4096, Epochs=args.epochs,
                  RandomizeStart=1, LearnLogStd=1, LogStdAlpha=1e-2, EntropyCoef=0.0)
    rows = []
    for it in range(20):
        e.rollout(args.horizon)
        z2 = e.log_std_gradient()["z2_mean"]
        e.ppo_update(update_index=it)
        s = e.log_std()
        ev = e.evaluate()
        rows.append({"iteration": it, "log_std": s["log_std"], "z2_mean_before_update": z2,
                     "grad_last": s["grad_last"], "eval_reward_mean": ev["reward_mean"]})
        print(json.dumps(rows[-1]), flush=True)
    e.close()
    return {"walkers": 4096, "LogStdAlpha": 1e-2, "EntropyCoef": 0.0, "iterations": rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=65536)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--minibatch", type=int, default=65536)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--bench-runs", type=int, default=3)
    p.add_argument("--bench-steps", type=int, default=10)
    p.add_argument("--bench-warmup", type=int, default=3)
    p.add_argument("--parent-root", default="")
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_std.json"))
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        return worker(args)
    if args.calls < 20:
        p.error("--calls: at least 20 per figure")
    wk = load(ROOT)
    res = {"shape": {"walkers": args.walkers, "horizon": args.horizon, "rows": args.walkers * args.horizon,
                     "minibatch": args.minibatch, "epochs": args.epochs,
                     "minibatches_per_epoch": args.walkers * args.horizon // args.minibatch},
           "clock": "host clock around synchronised calls"}
    res["update"] = time_arms(wk, args)
    print(json.dumps({"update": res["update"]}), flush=True)
    if args.parent_root:
        trees = {"this": ROOT, "parent": os.path.abspath(args.parent_root)}
        res["off_path_vs_parent"] = time_parent_update(args, trees)
        print(json.dumps({"off_path_vs_parent": res["off_path_vs_parent"]}), flush=True)
        if args.bench_runs > 0:
            res["bench_headline"] = time_parent_bench(args, trees)
    res["training_trace"] = training_trace(wk, args)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
