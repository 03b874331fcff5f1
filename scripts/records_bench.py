"""What the record exchange (wk_comm_records) costs on one GPU, at bench.py's shape (65,536 walkers,
T_h 64, M 65,536, 5 epochs): a measurement, no threshold.

Two contexts from the same seed, both with reward normalisation, TargetKL (a target nothing
reaches: every epoch runs) and LearnLogStd on, are alternated: `solo` has no communicator, `records`
has wk_comm_records(NULL) + wk_comm_init(0, 1, uid), a one-rank RCCL communicator.  Every timed
iteration restores the context's snapshot, then runs one wk_rollout and one wk_ppo_update at profile
level 1 (HIP events around the returns slot's launch groups and around the whole update).  Reported:

  returns_ms  per rollout: on `records` the reward normalisation's finish step is k_rnorm_batch, one
              ncclAllGather of 16 words and k_rnorm_merge instead of k_rnorm_finish
  update_ms   per update: on `records` every epoch's statistics record goes through k_record_pack
              and one ncclAllGather before the copy to the host the pass makes anyway -- and, as on
              every context with a communicator, every minibatch runs reduction, ncclAllReduce and
              Adam as three launches instead of one, which is not the record exchange's doing

The one-rank figure is an upper bound on what the feature adds on one GPU (RCCL's launch overhead
without any transfer).  What xGMI adds on eight GPUs is not measured here.

  python scripts/records_bench.py [--iters 20] [--warmup 3] [--out profiles/records.json]
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
    return {"returns_ms": p["returns_ms"], "update_ms": p["update_ms"], "physics_ms": p["physics_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20250905)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records.json"))
    args = ap.parse_args()
    import torch
    import wk
    if not torch.cuda.is_available():
        sys.exit("records_bench.py needs a GPU")

    engines = {}
    for name in ("solo", "records"):
        e = wk.Engine(args.walkers, seed=args.seed, Horizon=args.horizon, Minibatch=args.minibatch,
                      Epochs=args.epochs, RandomizeStart=1, TargetKL=1e30, LearnLogStd=1, EntropyCoef=0.01)
        if name == "records":
            e.comm_records(None)
            e.comm_init(0, 1, wk.Engine.comm_unique_id())
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
    keys = ("returns_ms", "update_ms", "physics_ms")
    out = {"shape": {k: getattr(args, k) for k in ("walkers", "horizon", "minibatch", "epochs", "iters", "warmup", "seed")},
           "device": torch.cuda.get_device_name(0)}
    for name in engines:
        out[name] = {k: spread([r[k] for r in runs[name]]) for k in keys}
    for k in keys:  # paired: iteration i of the one against iteration i of the other
        out["records_minus_solo_" + k] = spread([a[k] - b[k] for a, b in zip(runs["records"], runs["solo"])])
    same = all(engines["solo"].reward_norm_state()[k] == engines["records"].reward_norm_state()[k]
               for k in ("count", "mean", "m2", "scale"))
    out["same_statistics"] = same and engines["solo"].log_std() == engines["records"].log_std()
    out["figure"] = (f"returns slot {out['solo']['returns_ms']['median']:.3f} -> {out['records']['returns_ms']['median']:.3f} ms "
                     f"per rollout, update {out['solo']['update_ms']['median']:.3f} -> "
                     f"{out['records']['update_ms']['median']:.3f} ms (medians of {args.iters} runs; one-rank RCCL "
                     f"communicator against no communicator)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("figure", "records_minus_solo_returns_ms", "records_minus_solo_update_ms",
                                          "same_statistics")}))
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
