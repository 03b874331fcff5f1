"""What reward normalisation costs (k_rnorm_scan / k_rnorm_finish / k_rnorm_apply,
csrc/wk_rnorm.hip), one GPU, at bench.py's shape (65,536 walkers, T_h 64, M 65,536, 5 epochs).

Two contexts from the same seed, one enabled (wk_reward_norm_config) and one never enabled, are
alternated.  Every timed iteration restores the context's snapshot (walkers, weights, Adam, and on
the enabled context acc and the running statistics), then runs one wk_rollout and one
wk_ppo_update at profile level 1: HIP events on the context's stream around the physics launch,
around each launch group of the returns slot (episode log, the normalisation's three launches,
returns) and around the whole update.  The figure is the enabled-minus-disabled difference of the
returns slot per rollout, with the spread of the runs: the median of each side, the paired
differences' median, minimum and maximum.  The expectation from traffic (about 17 bytes per row
over 4.2 M rows) is tens of microseconds.

  python scripts/reward_norm_bench.py [--iters 30] [--warmup 3] [--out profiles/reward_norm.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-bipedalwalker_amd"))


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "stdev": statistics.pstdev(x),
            "runs": len(x)}


def iteration(e, horizon):
    e.restore()
    e.profile_reset()
    e.rollout(horizon)
    e.ppo_update(update_index=0, sync=False)
    p = e.profile()  # synchronises
    return {"returns_ms": p["returns_ms"], "physics_ms": p["physics_ms"], "update_ms": p["update_ms"],
            "returns_launches": p["returns_launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20250905)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_norm.json"))
    args = ap.parse_args()
    import torch
    import wk
    if not torch.cuda.is_available():
        sys.exit("reward_norm_bench.py needs a GPU")

    engines = {}
    for name in ("disabled", "enabled"):
        e = wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                      Epochs=args.epochs, RandomizeStart=1)
        if name == "enabled":
            e.reward_norm()
        e.rollout(args.horizon)  # (the regime bench.py times: one rollout in)
        e.snapshot()
        e.profile_enable(1)
        engines[name] = e
    runs = {name: [] for name in engines}
    for i in range(args.warmup + args.iters):
        for name, e in engines.items():
            r = iteration(e, args.horizon)
            if i >= args.warmup:
                runs[name].append(r)
    keys = ("returns_ms", "physics_ms", "update_ms")
    out = {"shape": {k: getattr(args, k) for k in ("walkers", "horizon", "minibatch", "epochs", "iters", "warmup", "seed")},
           "device": torch.cuda.get_device_name(0)}
    for name in engines:
        out[name] = {k: spread([r[k] for r in runs[name]]) for k in keys}
        out[name]["returns_launch_groups"] = runs[name][0]["returns_launches"]
    for k in keys:  # paired: iteration i of the one against iteration i of the other
        out["enabled_minus_disabled_" + k] = spread([a[k] - b[k] for a, b in zip(runs["enabled"], runs["disabled"])])
    st = engines["enabled"].reward_norm_state()
    out["state_after"] = {k: st[k] for k in ("count", "mean", "var", "scale", "rows", "clipped", "nonfinite")}
    d = out["enabled_minus_disabled_returns_ms"]
    out["figure"] = (f"returns slot: +{d['median'] * 1e3:.1f} us per rollout (paired differences "
                     f"{d['min'] * 1e3:.1f} .. {d['max'] * 1e3:.1f} us over {d['runs']} runs), beside a physics launch of "
                     f"{out['disabled']['physics_ms']['median']:.2f} ms")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("figure", "enabled_minus_disabled_returns_ms",
                                          "enabled_minus_disabled_physics_ms", "enabled_minus_disabled_update_ms")}))
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
