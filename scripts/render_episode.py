"""Frames of an episode, and what they cost.

Default: reset, then the first K walkers play one episode under the actor's mean action
(get_obs -> policy_sample -> step), every env-step rendered on the device with `follow`
(wk_render).  Writes every frame and a contact sheet (rows: walkers, columns: evenly spaced
env-steps) under --out: PNG through PIL when it imports, .npy otherwise.

  python scripts/render_episode.py [--walkers 4] [--n-env 64] [--weights critic.txt actor.txt]
                                   [--max-steps 1001] [--out frames]

--bench: wk_render_device alone, one GPU, at two shapes -- 64 views of the default frame (550 x
325, the whole floor) and 4,096 views of 96 x 96 at scale 0.25 with follow (image observations) --
timed with the host clock around a burst of back-to-back calls that ends in a stream synchronise
(a warm-up first; the burst is sized to last about --window seconds; --calls bursts, every figure
with its spread), beside the only earlier way to reach the geometry: the wk_get_body_view loop
over the same walkers (5 bodies and the floor each, one synchronise and one copy per call), which
fetches vertices and draws nothing.  Writes profiles/render.json.

  python scripts/render_episode.py --bench [--calls 5] [--window 0.5] [--out profiles/render.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-bipedalwalker_amd"))
import wk  # noqa: E402

FOLLOW = dict(width=256, height=160, scale=1.0, follow=1, ox=0.0, oy=759.5)  # the floor on row 140's centres
SHAPES = {
    "default_frame_64_views": (64, dict()),
    "obs_96x96_4096_views": (4096, dict(width=96, height=96, scale=0.25, follow=1, ox=0.0, oy=598.0)),
}


def spread(v, unit="ms"):
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v),
            f"stdev_{unit}": statistics.pstdev(v), "calls": len(v)}


def save_image(path, img):
    """RGBA uint8 [H, W, 4] as PNG when PIL imports, else as .npy; returns the path written"""
    try:
        from PIL import Image
    except ImportError:
        np.save(path + ".npy", img)
        return path + ".npy"
    Image.fromarray(img, "RGBA").save(path + ".png")
    return path + ".png"


def episode(args):
    eng = wk.Engine(args.n_env, seed=args.seed, RandomizeStart=1)
    if args.weights:
        eng.load_weights(*args.weights)
    eng.reset()
    k = min(args.walkers, eng.n)
    ids = list(range(k))
    alive = np.ones(k, bool)
    frames = [eng.render(ids, **FOLLOW)]
    for t in range(args.max_steps):
        mean, _, _ = eng.policy_sample(eng.get_obs())
        _, _, done, _ = eng.step(mean[None], 1)
        alive &= ~done[0, :k].astype(bool)
        if not alive.any():
            break  # (the step that ended the last episode has already reset its walker)
        frames.append(eng.render(ids, marker_x=float(eng.get_state()[:k, wk.ST_POS].max()), **FOLLOW))
    eng.close()
    frames = np.stack(frames)  # [t, k, H, W, 4]
    os.makedirs(args.out, exist_ok=True)
    for t in range(frames.shape[0]):
        for i in ids:
            save_image(os.path.join(args.out, f"walker{i:03d}_step{t:04d}"), frames[t, i])
    cols = np.unique(np.linspace(0, frames.shape[0] - 1, min(8, frames.shape[0])).astype(int))
    sheet = np.concatenate([np.concatenate([frames[t, i] for t in cols], axis=1) for i in ids], axis=0)
    where = save_image(os.path.join(args.out, "contact_sheet"), sheet)
    print(json.dumps({"env_steps": int(frames.shape[0] - 1), "walkers": k, "frame": list(frames.shape[2:4]),
                      "lit_fraction": float((frames[..., :3] != 0).any(axis=-1).mean()), "contact_sheet": where}))


def bench_shape(args, name, n_views, kw):
    import torch
    eng = wk.Engine(max(n_views, 64), seed=args.seed, RandomizeStart=1)
    eng.step(None, 8)  # walkers in motion: live torques, distinct poses
    ids = list(range(n_views))
    a = wk.render_args(**kw)
    nbytes = n_views * a.height * a.width * 4
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr()

    def burst(reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.render_device(ptr, ids, **kw)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    burst(3)  # warm: the code object, the id buffer
    reps = max(8, int(args.window * 1e3 / max(burst(8), 1e-3)))
    device_ms = [burst(reps) for _ in range(args.calls)]
    img = buf.cpu().numpy().reshape(n_views, a.height, a.width, 4)
    # the earlier way: the geometry of the same walkers through the per-body getter
    def getter_loop():
        t0 = time.perf_counter()
        for e in ids:
            for b in range(6):
                eng.body_view(e, b)
        return (time.perf_counter() - t0) * 1e3

    getter_loop()  # warm
    getter_ms = [getter_loop() for _ in range(args.calls)]
    # and the host-image variant: the same frames copied out (one call, synchronous)
    t0 = time.perf_counter()
    host = eng.render(ids, **kw)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert host.tobytes() == img.tobytes()
    eng.close()
    out = {"views": n_views, "frame": [a.width, a.height], "args": {k: v for k, v in a.as_dict().items() if k != "marker_x"},
           "image_bytes": nbytes, "burst": reps,
           "render_device": spread(device_ms),
           "lit_fraction": float((img[..., :3] != 0).any(axis=-1).mean()),
           "body_view_loop": dict(spread(getter_ms), calls_per_pass=6 * n_views,
                                  note="vertices only: 5 bodies and the floor per walker, nothing drawn"),
           "render_to_host_once_ms": host_ms}
    med = out["render_device"]["median_ms"]
    out["views_per_s"] = n_views / (med * 1e-3)
    out["image_gb_per_s"] = nbytes / (med * 1e-3) / 1e9
    out["body_view_loop_over_render_device"] = out["body_view_loop"]["median_ms"] / med
    print(json.dumps({name: out}), flush=True)
    return out


def bench(args):
    res = {"clock": "host clock around a burst of wk_render_device calls ending in a stream synchronise, per call; "
                    "the body_view loop: host clock around the synchronous getters",
           "kernel": "k_render: one block of 256 threads per 64 x 16 tile of one view"}
    for name, (n_views, kw) in SHAPES.items():
        res[name] = bench_shape(args, name, n_views, kw)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--bench", action="store_true")
    p.add_argument("--walkers", type=int, default=4)
    p.add_argument("--n-env", type=int, default=64)
    p.add_argument("--weights", nargs=2, metavar=("CRITIC", "ACTOR"))
    p.add_argument("--max-steps", type=int, default=1001)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--window", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=20250905)
    p.add_argument("--out")
    args = p.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "render.json") if args.bench else "frames"
    bench(args) if args.bench else episode(args)


if __name__ == "__main__":
    main()
