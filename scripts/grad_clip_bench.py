"""What MaxGradNorm costs (k_clip_adam, csrc/wk_tail.hip), one GPU, at bench.py's shape (65,536
walkers, T_h 64, M 65,536, 5 epochs: 320 Adam steps per update).

  1. wk_ppo_update with MaxGradNorm in {0, inf, 0.5} on the built-in kernels and on the general
     kernels with the default strings: every timed update starts from the context's snapshot and
     is timed with the host clock around synchronised calls, the three contexts alternated; then
     one untimed update at profile level 2 gives the mean per-launch reduce and Adam times (an
     event pair around every launch).
  2. the k_clip_adam launch alone on the widest general network (netref.NETS["max"], 70,021
     parameters): the level-2 Adam slot of a small update on such a context.
  3. the off path against the parent commit, with --parent-root DIR (a built checkout of the
     parent): the MaxGradNorm = 0 update of this tree and the parent's update, alternated, every
     run a fresh process (--runs of them, at least 5, each the median of --calls updates).  The
     margin is the spread of the parent's own runs.

  python scripts/grad_clip_bench.py [--calls 20] [--runs 5] [--parent-root DIR]
                                    [--out profiles/grad_clip.json]
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
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, os.path.join(root, "ppo-bipedalwalker_amd"))
    import wk
    return wk


def engine(wk, args, kernels, max_norm):
    cfg = dict(Horizon=args.horizon, Minibatch=args.minibatch, Epochs=args.epochs, RandomizeStart=1,
               NetworkKernels=kernels)
    if max_norm:  # (the parent commit has no such field)
        cfg["MaxGradNorm"] = max_norm
    return wk.Engine(args.walkers, seed=args.seed, **cfg)


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


def launches(e):
    """mean microseconds per reduce and per Adam launch of one update (profile level 2)"""
    e.restore()
    e.profile_reset()
    e.profile_enable(2)
    e.ppo_update(update_index=0)
    p = e.profile()
    e.profile_enable(0)
    per = lambda ms, n: ms / n * 1e3 if n else None
    return {"grad_launches": p["grad_launches"], "reduce_launches": p["reduce_launches"],
            "adam_launches": p["adam_launches"], "grad_us": per(p["grad_ms"], p["grad_launches"]),
            "reduce_us": per(p["reduce_ms"], p["reduce_launches"]),
            "adam_us": per(p["adam_ms"], p["adam_launches"])}


def time_family(wk, args, kernels):
    norms = {"0": 0.0, "inf": float("inf"), "0.5": 0.5}
    engs = {k: engine(wk, args, kernels, v) for k, v in norms.items()}
    for e in engs.values():
        prepare(e, args)
    ms = {k: [] for k in engs}
    for _ in range(args.calls):
        for k, e in engs.items():
            ms[k].append(timed_update(e))
    out = {}
    for k, e in engs.items():
        out[k] = spread(ms[k])
        out[k]["per_launch"] = launches(e)
        if k != "0":
            g = e.grad_norms()
            out[k]["record"] = {"steps": g["steps"], "clipped": g["clipped"], "nonfinite": g["nonfinite"],
                                "norm_max": g["norm_max"]}
        e.close()
    steps = args.epochs * (args.walkers * args.horizon // args.minibatch)
    for k in ("inf", "0.5"):
        out[k]["us_per_minibatch_over_off"] = (out[k]["median_ms"] - out["0"]["median_ms"]) / steps * 1e3
    return out


def time_clip_alone(wk, args):
    import netref
    c, a = netref.NETS["max"]
    e = wk.Engine(256, seed=args.seed, Horizon=4, Minibatch=64, Epochs=4, NetworkKernels=1,
                  CriticNeuralNetwork=c, ActorNeuralNetwork=a, MaxGradNorm=0.5)
    e.rollout(4)
    e.snapshot()
    e.ppo_update(update_index=0)
    us = []
    for _ in range(args.calls):
        us.append(launches(e)["adam_us"])
    out = {"network": "max", "parameters": e.nparam, "launches_per_sample": 64, "clock": "an event pair around each launch",
           "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}
    e.close()
    return out


def worker(args):
    """one fresh process: the median of --calls MaxGradNorm = 0 updates of the tree at --tree"""
    wk = load(args.tree)
    e = engine(wk, args, 0, 0.0)
    prepare(e, args)
    ms = [timed_update(e) for _ in range(args.calls)]
    e.close()
    print(json.dumps(spread(ms)))


def time_parent(args):
    trees = {"this": ROOT, "parent": os.path.abspath(args.parent_root)}
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
    out = {"what": "wk_ppo_update, MaxGradNorm = 0 (this tree) against the parent commit; every run a fresh "
                   "process, its figure the median of --calls updates from the snapshot",
           "runs": args.runs}
    for k, v in runs.items():
        out[k] = {"median_ms_per_run": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    out["parent_spread_ms"] = out["parent"]["max"] - out["parent"]["min"]
    out["this_minus_parent_ms"] = out["this"]["median"] - out["parent"]["median"]
    out["within_parent_spread"] = abs(out["this_minus_parent_ms"]) <= out["parent_spread_ms"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=65536)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--minibatch", type=int, default=65536)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--parent-root", default="")
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.json"))
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        return worker(args)
    if args.parent_root and args.runs < 5:
        p.error("--runs: at least 5 per tree")
    wk = load(ROOT)
    res = {"shape": {"walkers": args.walkers, "horizon": args.horizon, "minibatch": args.minibatch,
                     "epochs": args.epochs, "adam_steps": args.epochs * (args.walkers * args.horizon // args.minibatch)},
           "clock": "host clock around synchronised calls; per_launch: an event pair around every launch"}
    for name, kernels in (("builtin", 0), ("general_default", 1)):
        res[f"update_{name}"] = time_family(wk, args, kernels)
        print(json.dumps({f"update_{name}": res[f"update_{name}"]}), flush=True)
    res["clip_adam_alone"] = time_clip_alone(wk, args)
    print(json.dumps({"clip_adam_alone": res["clip_adam_alone"]}), flush=True)
    if args.parent_root:
        res["off_path_vs_parent"] = time_parent(args)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
