"""GPU, two and three processes sharing GPU 0: TargetKL, LearnLogStd and reward normalisation over
the record exchange (wk_comm_records).  The gradients go through wk_comm_init_host and gloo, the
statistics records through wk.dist.gather_records (tests/workers/records_worker.py); each rank holds
272 walkers (EnvOffset = rank x 272) over a horizon of 11.  Checked, to the byte where the design
promises bytes:

  * every rank holds the same global sums, and they are the ranks' local sums folded in rank order
    (with three ranks another order gives other bytes); the update's record is their division;
  * the stop decision is the global one: a target between the global kl and the largest local kl
    stops nobody after epoch 1, and every rank runs the same number of epochs;
  * the log-std is the same on every rank, is the host Adam step on the global gradient, and is not
    what a rank alone on its shard reaches;
  * the reward normalisation's statistics are the same on every rank, count every shard's samples,
    match numpy float64 over all shards' samples within the summation bound, scale each shard's
    rewards by the global scale, and differ from a lone shard's;
  * weights and Adam state stay replicas.
"""
import itertools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import logstdref
import rnormref
import sumsref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 272, 11
ENTROPY = 0.01


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(out, n):
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(
            ["timeout", "-k", "10", "240", sys.executable,
             os.path.join(ROOT, "tests", "workers", "records_worker.py"), str(out)],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    ranks = []
    for r in range(n):
        z = np.load(out / f"rank{r}.npz")
        d = {k: z[k] for k in z.files if k != "meta"}
        d["meta"] = json.loads(str(z["meta"]))
        ranks.append(d)
    return ranks


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """one run with two ranks and one with three: at most three processes with the GPU open"""
    return {n: _run_ranks(tmp_path_factory.mktemp(f"records{n}"), n) for n in (2, 3)}


def _sums(wk, a):
    return wk.PpoSums.from_buffer_copy(a.tobytes()).as_dict()


def _fold(wk, recs):
    acc = recs[0]
    for r in recs[1:]:
        acc = wk.sums_add(acc, r)
    return acc


def _eq(a, b, keys):
    """equal values, a NaN equal to a NaN (one side went through JSON, which keeps no NaN payload)"""
    return all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in keys)


def _same(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # (repr round-trips doubles)


@pytest.mark.parametrize("world", [2, 3])
def test_global_sums_are_the_rank_ordered_fold(wk, runs, world):
    rs = runs[world]
    differs = False
    for u in (0, 1):
        k = f"multi{u}_"
        for r in rs[1:]:
            assert r[k + "global"].tobytes() == rs[0][k + "global"].tobytes(), (u, "global sums differ between ranks")
        local = [_sums(wk, r[k + "local"]) for r in rs]
        glo = _sums(wk, rs[0][k + "global"])
        assert sumsref.same_bytes(glo, _fold(wk, local), sumsref.FIELDS)
        assert sumsref.same_bytes(glo, sumsref.fold(local), sumsref.FIELDS)
        assert glo["rows"] + glo["skipped"] == world * N * T
        assert len({r[k + "local"].tobytes() for r in rs}) == world  # the shards differ
        # the update's record is the division of the global sums (the pass ran once: epoch 1 of 1)
        want = dict(wk.stats_from_sums(glo), epochs_run=1, stopped_early=0)
        for r in rs:
            assert _eq(r["meta"][k + "upd"], want, sumsref.STATS_KEYS), (u, r["meta"][k + "upd"], want)
        for order in itertools.permutations(range(world)):
            if order != tuple(range(world)):
                differs |= not sumsref.same_bytes(glo, _fold(wk, [local[i] for i in order]), sumsref.FIELDS)
    if world == 3:
        assert differs, "every order of the fold gives the same bytes on this data: the rank order is not pinned"


@pytest.mark.parametrize("world", [2, 3])
def test_the_stop_decision_is_the_global_one(runs, world):
    rs = runs[world]
    m0 = rs[0]["meta"]["run2"]
    kg, kmax, target = m0["kl_global"], max(m0["kl_all"]), m0["target"]
    for i, r in enumerate(rs):
        assert _same(r["meta"]["run2"]["kl_all"], m0["kl_all"]) and r["meta"]["run2"]["target"] == target
        assert r["meta"]["run2"]["kl_local"] == m0["kl_all"][i]
    # the premise: some rank's own kl is past the target while the global one is not
    assert kg < target < kmax, f"local kl {m0['kl_all']} and global kl {kg} leave no room for a target between them"
    for r in rs:
        u = r["meta"]["run2_upd"]
        assert u["epochs_run"] >= 2, u
        assert _same(u, rs[0]["meta"]["run2_upd"])
        assert r["meta"]["run2_t"] == rs[0]["meta"]["run2_t"] == u["epochs_run"]  # one minibatch per epoch
        assert _same(r["meta"]["run2_ls"], rs[0]["meta"]["run2_ls"])
        for k in ("run2_w", "run2_m", "run2_v"):
            assert r[k].tobytes() == rs[0][k].tobytes(), k


@pytest.mark.parametrize("world", [2, 3])
def test_log_std_steps_on_the_global_gradient(wk, runs, world):
    rs = runs[world]
    cfg = wk.default_config()
    for u in (0, 1):
        k = f"multi{u}_"
        for r in rs:
            assert _same(r["meta"][k + "ls1"], rs[0]["meta"][k + "ls1"]), (u, "the log-std differs between ranks")
        ls0, ls1 = rs[0]["meta"][k + "ls0"], rs[0]["meta"][k + "ls1"]
        g = wk.log_std_grad_from_sums(_sums(wk, rs[0][k + "global"]), ENTROPY)
        assert g["grad"] == ls1["grad_last"]
        s, m, v, t, clamped, stepped = logstdref.adam_scalar(
            ls0["log_std"], ls0["m"], ls0["v"], ls0["t"], g["grad"], float(cfg.Alpha), float(cfg.Beta1),
            float(cfg.Beta2), float(cfg.AdamEpsilon), float(cfg.LogStdMin), float(cfg.LogStdMax))
        assert stepped and (s, m, v, t) == (ls1["log_std"], ls1["m"], ls1["v"], ls1["t"])
        # a rank alone on its shard steps on its own gradient and lands elsewhere
        solo = rs[0]["meta"][f"solo{u}_ls1"]
        assert solo["t"] == ls1["t"] and (solo["log_std"], solo["m"]) != (ls1["log_std"], ls1["m"])
        g_solo = wk.log_std_grad_from_sums(_sums(wk, rs[0][f"solo{u}_local"]), ENTROPY)
        assert g_solo["grad"] == solo["grad_last"] != g["grad"]


@pytest.mark.parametrize("world", [2, 3])
def test_reward_normalisation_uses_every_shard(wk, runs, world):
    rs = runs[world]
    gamma = float(wk.default_config().Gamma)
    acc = [None] * world
    xs = []
    for u in (0, 1):
        k = f"multi{u}_"
        st = rs[0]["meta"][k + "rnorm"]
        for r in rs:
            for f in ("count", "mean", "m2", "var", "scale", "nonfinite"):
                assert _same(r["meta"][k + "rnorm"][f], st[f]), (u, f)
        bad = 0
        for i, r in enumerate(rs):
            acc[i], x, b = rnormref.scan(r[k + "rewards"], r[k + "dones"], gamma, acc[i])
            xs += x
            bad += b
        x64 = np.array(xs, np.float64)
        assert st["count"] == x64.size and st["nonfinite"] == bad == 0
        # two differently associated double sums of N terms differ by at most 2 (N - 1) u sum|x|
        u53, n = 2.0 ** -53, x64.size
        mean = float(np.mean(x64))
        assert abs(st["mean"] - mean) <= 2 * n * u53 * float(np.abs(x64).sum()) / n
        assert abs(st["m2"] - float(((x64 - mean) ** 2).sum())) <= 4 * n * u53 * float((x64 * x64).sum())
        var, scale = rnormref.scale_of(st["count"], st["m2"], st["epsilon"])
        assert st["var"] == var and np.float32(st["scale"]) == scale
        for i, r in enumerate(rs):
            want, clipped = rnormref.apply(r[k + "rewards"], np.float32(st["scale"]), st["clip"])
            assert r[k + "scaled"].tobytes() == want.tobytes(), (u, i)
            assert r["meta"][k + "rnorm"]["clipped"] == clipped and r["meta"][k + "rnorm"]["rows"] == N * T
        solo = rs[0]["meta"][f"solo{u}_rnorm"]
        assert solo["count"] < st["count"] and solo["scale"] != st["scale"]


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_stay_identical(runs, world):
    rs = runs[world]
    for u in (0, 1):
        for k in ("w", "m", "v"):
            for r in rs[1:]:
                assert r[f"multi{u}_{k}"].tobytes() == rs[0][f"multi{u}_{k}"].tobytes(), (u, k)
        assert len({r["meta"][f"multi{u}_t"] for r in rs}) == 1
        assert rs[0][f"multi{u}_w"].tobytes() != rs[0][f"solo{u}_w"].tobytes()
    assert rs[0]["meta"]["multi1_t"] == 2 and rs[0]["multi0_w"].tobytes() != rs[0]["multi1_w"].tobytes()
