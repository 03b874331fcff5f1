"""What the policy statistics cost (wk_policy_stats, the TargetKL check), one GPU, at bench.py's
shape (65,536 walkers, T_h 64: 4.19 M rows; M 65,536, 5 epochs).  A warm-up, then at least 20
calls per figure, timed with the host clock around synchronised calls; every figure is recorded
with its spread (median, min, max, standard deviation).

  1. wk_policy_stats per call on a built-in context and on a general one (default strings), as
     achieved TFLOP/s on the counted flops -- 2 * sum(out * in) per row, the forward's
     multiply-adds -- and the share of the 157.3 TFLOP/s fp32 matrix-core peak, beside the rows'
     bytes against 8 TB/s.
  2. wk_ppo_update with TargetKL = 1e9 (a check after every epoch, never a stop) against
     TargetKL = 0 on the same build, alternated A B A B, each from the same snapshot.
  3. with --parent-root DIR (a built checkout of the parent commit): `python bench.py`'s headline
     of this tree against that one, alternated, each run a fresh process.

  python scripts/policy_stats_bench.py [--calls 20] [--bench-runs 3] [--parent-root DIR]
                                       [--out profiles/policy_stats.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ppo-bipedalwalker_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import wk  # noqa: E402
import netref  # noqa: E402

PEAK_TFLOPS = 157.3
HBM_TBS = 8.0
ROW_BYTES = 4 * (12 + 4 + 4 + 1 + 1)  # state, action, logp_old, return, advantage


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "stdev_ms": statistics.pstdev(ms), "calls": len(ms)}


def flop_per_row(critic, actor):
    return 2 * sum(i * o for dsl in (critic, actor) for k, i, o in netref.layers(dsl) if k == "D")


def engine(args, kernels, **cfg):
    return wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                     Epochs=args.epochs, RandomizeStart=1, NetworkKernels=kernels, **cfg)


def time_stats(args, kernels):
    eng = engine(args, kernels)
    eng.rollout(args.horizon)
    eng.ppo_update(update_index=0)  # a policy that has moved
    eng.sync()
    for _ in range(3):
        st = eng.policy_stats()
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        eng.policy_stats()
        ms.append((time.perf_counter() - t0) * 1e3)
    rows = st["samples"] + st["skipped"]
    flop = flop_per_row(netref.CRITIC_DEFAULT, netref.ACTOR_DEFAULT) * rows
    out = spread(ms)
    sec = out["median_ms"] * 1e-3
    out.update(rows=rows, flop_per_row=flop // rows, tflops=flop / sec / 1e12,
               fraction_of_fp32_mfma_peak=flop / sec / 1e12 / PEAK_TFLOPS,
               row_bytes=ROW_BYTES, tb_per_s=rows * ROW_BYTES / sec / 1e12,
               fraction_of_hbm_peak=rows * ROW_BYTES / sec / 1e12 / HBM_TBS,
               stats={k: st[k] for k in ("kl", "kl_k1", "clip_fraction", "ratio_max", "explained_variance")})
    eng.close()
    return out


def time_update(args, kernels):
    """A = TargetKL 0, B = TargetKL 1e9, alternated; each update from its context's snapshot"""
    engs = {"off": engine(args, kernels), "check": engine(args, kernels, TargetKL=1e9)}
    for e in engs.values():
        e.rollout(args.horizon)
        e.snapshot()
        e.ppo_update(update_index=0, sync=False)  # warm
        e.sync()
    ms = {"off": [], "check": []}
    for _ in range(args.calls):
        for k, e in engs.items():
            e.restore()
            e.sync()
            t0 = time.perf_counter()
            e.ppo_update(update_index=0, sync=False)
            e.sync()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    us = engs["check"].update_stats()
    out = {k: spread(v) for k, v in ms.items()}
    out["checks_per_update"] = us["epochs_run"]
    per_check = (out["check"]["median_ms"] - out["off"]["median_ms"]) / max(1, us["epochs_run"])
    out["ms_per_check"] = per_check
    out["ms_per_epoch_off"] = out["off"]["median_ms"] / args.epochs
    out["check_over_epoch"] = per_check / out["ms_per_epoch_off"]
    for e in engs.values():
        e.close()
    return out


def bench_headline(root, args):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps),
                        "--warmup", str(args.bench_warmup)], cwd=root, capture_output=True, text=True,
                       timeout=900, check=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    return {"value": d["value"], "ms_per_step": d["ms_per_step"]}


def time_bench(args):
    trees = {"this": ROOT}
    if args.parent_root:
        trees["parent"] = os.path.abspath(args.parent_root)
    runs = {k: [] for k in trees}
    for _ in range(args.bench_runs):
        for k, root in trees.items():
            runs[k].append(bench_headline(root, args))
            print(json.dumps({k: runs[k][-1]}), flush=True)
    out = {"command": f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}"}
    for k, v in runs.items():
        vals = [x["value"] for x in v]
        out[k] = {"env_steps_per_s": vals, "median": statistics.median(vals), "min": min(vals), "max": max(vals),
                  "ms_per_step": [x["ms_per_step"] for x in v]}
    if "parent" in out:
        out["this_over_parent"] = out["this"]["median"] / out["parent"]["median"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=65536)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--minibatch", type=int, default=65536)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--bench-runs", type=int, default=3)
    p.add_argument("--bench-steps", type=int, default=10)
    p.add_argument("--bench-warmup", type=int, default=3)
    p.add_argument("--parent-root", default="")
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_stats.json"))
    args = p.parse_args()
    if args.calls < 20:
        p.error("--calls: at least 20 per figure")
    res = {"shape": {"walkers": args.walkers, "horizon": args.horizon, "rows": args.walkers * args.horizon,
                     "minibatch": args.minibatch, "epochs": args.epochs},
           "clock": "host clock around synchronised calls"}
    for name, kernels in (("builtin", 0), ("general_default", 1)):
        res[f"policy_stats_{name}"] = time_stats(args, kernels)
        print(json.dumps({f"policy_stats_{name}": res[f"policy_stats_{name}"]}), flush=True)
    for name, kernels in (("builtin", 0), ("general_default", 1)):
        res[f"update_{name}"] = time_update(args, kernels)
        print(json.dumps({f"update_{name}": res[f"update_{name}"]}), flush=True)
    if args.bench_runs > 0:
        res["bench_headline"] = time_bench(args)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
