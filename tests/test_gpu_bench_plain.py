"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run end to end -- one JSON line with the
headline keys and nothing that takes runs of its own (no CPU baseline, rooflines, other shapes or
detail file: those go with `--full`), and `--dump-outputs DIR`: the files hold what the last
timed step computed, checked bit for bit against the same sequence (regime iteration, snapshot,
then restore + rollout + PPO update) driven through the engine in this process.  Small shapes:
8,192 walkers (the 8-GPU shard; twice the dumped sample of 4,096 walkers), T = 8, one epoch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250905  # bench.py's default --seed
N, T, STEPS, WARMUP = 8192, 8, 3, 1


def test_plain_run_line_and_dumped_outputs(wk, tmp_path):
    d = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--walkers-global", str(N), "--horizon", str(T), "--epochs", "1",
           "--regime-iters", "1", "--dump-outputs", str(d)]
    p = subprocess.run(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out, k
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["dtype"] == "f32"
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - N * T / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    for k in ("cpu_baseline", "configs", "roofline", "roofline_update", "detail_file"):
        assert k not in out, k
    assert os.listdir(tmp_path) == ["out"]  # nothing else written

    # the same sequence in this process: what the last timed step left in the engine
    eng = wk.Engine(N, seed=SEED, Horizon=T, Minibatch=N, MinibatchGlobal=N, Epochs=1,
                    RandomizeStart=1)
    try:
        eng.rollout(T)
        eng.ppo_update(update_index=0, sync=False)
        eng.snapshot()
        eng.restore()
        eng.rollout(T)
        eng.ppo_update(update_index=1, sync=False)
        eng.sync()
        m, v, t = eng.get_adam()
        want = {"weights": eng.get_weights(), "adam_m": m, "adam_v": v, "adam_t": np.array([t])}
        state, traj = eng.get_state(), eng.get_trajectory(T)
    finally:
        eng.close()
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert set(got) == set(want) | {"walkers", "state"} | {"trajectory_" + k for k in traj}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["walkers"].astype(np.int64)
    assert len(idx) == 4096 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < N
    want["state"] = state[idx]
    for k, a in traj.items():
        want["trajectory_" + k] = a[:, idx]
    for k, a in want.items():
        assert np.array_equal(got[k], a.astype(np.float32), equal_nan=True), k
    # two updates (the regime's and the timed step's) of N * T / N = T minibatches each
    assert np.isfinite(got["weights"]).all() and got["adam_t"][0] == 2 * T
    assert got["trajectory_states"].shape == (T, len(idx), 12)
