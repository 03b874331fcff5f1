"""A first learning record for ReturnsMode: the reference's returns (0: the GAE chain never carried,
every horizon cut scanned from 0) against the standard estimators (1: chained GAE(Lambda), the
critic's value at the cut), each with UseGAE 0 and 1, on one GPU with the default networks --
4,096 walkers, Horizon 64, a few hundred rollout-and-update iterations, three seeds each.  Every
25 updates it records the mean total reward and the mean length of the episodes finished since
the last drain of the episode log (wk_episode_log_drain).  A record, not a test.

Then the cost at bench.py's shape (65,536 walkers x 64 steps; the snapshot restored before every
timed iteration, as bench.py does): wk_profile's physics_ms and returns_ms per rollout in both
modes.  returns_ms covers the episode log, the returns scan and, in mode 1, the two launches that
fill the bootstrap values.

  python scripts/returns_compare.py [--walkers N] [--iters K] [--every E] [--seeds a,b,c]
                                    [--minibatch M] [--part learn|cost|all]
                                    [--out profiles/returns_mode.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-bipedalwalker_amd"))
import wk  # noqa: E402


def learn(args, mode, gae, seed):
    eng = wk.Engine(args.walkers, seed=seed, Horizon=args.horizon, Minibatch=args.minibatch,
                    RandomizeStart=1, ReturnsMode=mode, UseGAE=gae)
    points = []
    for it in range(1, args.iters + 1):
        eng.rollout(args.horizon)
        eng.ppo_update(update_index=it - 1, sync=False)
        if it % args.every == 0:
            recs, dropped = eng.drain_episodes()
            eng.drain_losses()
            points.append({
                "update": it, "episodes": int(recs.size), "dropped": int(dropped),
                "mean_total_reward": float(recs["total_reward"].astype(np.float64).mean()) if recs.size else None,
                "mean_length": float(recs["length"].mean()) if recs.size else None})
    finite = bool(np.isfinite(eng.get_weights()).all())
    eng.close()
    return {"ReturnsMode": mode, "UseGAE": gae, "seed": seed, "weights_finite": finite, "points": points}


def cost(args, mode):
    eng = wk.Engine(args.cost_walkers, seed=args.cost_seed, Horizon=args.horizon, Minibatch=args.cost_walkers,
                    RandomizeStart=1, ReturnsMode=mode)
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
    iterations(args.cost_steps)
    p = eng.profile()
    eng.close()
    k = max(1, p["physics_launches"])
    return {"ReturnsMode": mode, "rollouts": p["physics_launches"], "physics_ms_per_rollout": p["physics_ms"] / k,
            "returns_ms_per_rollout": p["returns_ms"] / k, "returns_scopes_per_rollout": p["returns_launches"] / k,
            "update_ms": p["update_ms"] / max(1, p["update_calls"])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--walkers", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=64)
    p.add_argument("--minibatch", type=int, default=16384)
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--every", type=int, default=25)
    p.add_argument("--seeds", default="20250905,20250906,20250907")
    p.add_argument("--cost-walkers", type=int, default=65536)
    p.add_argument("--cost-steps", type=int, default=5)
    p.add_argument("--cost-seed", type=int, default=20250905)
    p.add_argument("--regime-iters", type=int, default=2)
    p.add_argument("--part", choices=["learn", "cost", "all"], default="all")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "returns_mode.json"))
    args = p.parse_args()
    seeds = [int(s) for s in args.seeds.split(",")]
    res = {"shape": {"walkers": args.walkers, "horizon": args.horizon, "minibatch": args.minibatch,
                     "epochs": 5, "iterations": args.iters, "every": args.every, "seeds": seeds,
                     "networks": "default", "Gamma": 0.9, "Lambda": 0.95}}
    if args.part in ("learn", "all"):
        res["learning"] = []
        for mode in (0, 1):
            for gae in (0, 1):
                for seed in seeds:
                    run = learn(args, mode, gae, seed)
                    res["learning"].append(run)
                    last = run["points"][-1] if run["points"] else {}
                    print(json.dumps({"ReturnsMode": mode, "UseGAE": gae, "seed": seed, "last": last}), flush=True)
    if args.part in ("cost", "all"):
        res["cost"] = {"shape": {"walkers": args.cost_walkers, "horizon": args.horizon,
                                 "timed_iterations": args.cost_steps},
                       "modes": [cost(args, 0), cost(args, 1)]}
        print(json.dumps(res["cost"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
