"""GPU: the trained log-std (LearnLogStd, EntropyCoef), wk_log_std_gradient, wk_get / wk_set_log_std
and wk_set_log_std_adam on the built-in kernels (k_ppo_logstd) and the general ones
(k_net_logstd) -- tests/logstdref.py holds the float64 restatement, tests/test_logstdref.py
checks it without a GPU.  Families, cases and sizes are tests/test_gpu_stats.py's: P = 1, 15, 16,
17, 33 and per family one row past a whole grid pass.  Every case prints its figures (pytest -s).

 (1) the reduction alone: log_std_gradient() against a float64 aggregation of logstdref.terms32
     on the kernel's own per-row lp (policy_stats(per_sample=True): the same forward, so the two
     passes' counts agree) and the buffer's fp32 logp_old and advantages.  |d sum term| <= 4 *
     2^-23 sum|term| (device and numpy expf may differ in the last place: test_gpu_stats' bar for
     the surrogate); counts exact.  z2_mean: the kernel forms zz = ((act - mean) / std)^2 and
     lp = lp_const - zz / 2, and only lp is an output, so the kernel's fp32 zz is known up to the
     rounding of that subtraction: every zz consistent with the observed lp lies in
     logstdref.zz_bracket.  z2_mean must lie within 2^-52 sum zz / N of the float64 means of the
     bracket's ends -- the bound on the reduction itself is the stated one, and nothing observable
     pins the fp32 zz closer.
 (2) end to end against grad64 with the per-row bar propagated: tau = 1e-5 max|lp64| + 2e-5,
     bound tau mean(|w| (|zz - 1| + 2)) + 4 tau^2 mean|w| (a ratio moves by r tau, zz = 2 (lp_const
     - lp) by 2 tau; no selection flips: every ratio is 1e-3 from a bound, test_statsref).
 (3) .. (11): see the tests.
"""
import math
import struct

import numpy as np
import pytest

import logstdref
import netref
import statsref
import test_gpu_stats as tgs

pytestmark = pytest.mark.gpu

SEED = tgs.SEED
F = np.float32
U52, U23 = 2.0 ** -52, 2.0 ** -23
FAMILIES = tgs.FAMILIES
CASES = [(fam, name, P) for fam, name in FAMILIES for P in statsref.SMALL_P + (statsref.large_p(fam),)]
TWO = [("builtin", "default"), ("general", "odd")]
LS_FLOATS = ("m", "v", "entropy", "grad_last")
LS_INTS = ("t", "steps", "clamped", "nonfinite")


def _gbytes(g):
    return (int(g["samples"]), int(g["skipped"])) + tuple(
        np.float64(g[k]).tobytes() for k in ("grad_surrogate", "grad", "z2_mean"))


def _lbytes(s, keys=LS_FLOATS + LS_INTS):
    return (F(s["log_std"]).tobytes(), F(s["std"]).tobytes()) + tuple(
        np.float64(s[k]).tobytes() if k in LS_FLOATS else int(s[k]) for k in keys)


def _put(wk, family, name, P, traj=None, eng=None, weights=None, **cfg):
    """an engine holding the case's weights and trajectory, and the buffer's fp32 logp_old / adv"""
    w, base = statsref.case(name, P)
    n, T = statsref.SHAPES[P]
    if eng is None:
        eng = tgs._engine(wk, family, name, n, T, **cfg)
    eng.set_weights(w if weights is None else weights)
    eng.set_trajectory(**(base if traj is None else traj))
    return eng


def _buffer(eng, P):
    n, T = statsref.SHAPES[P]
    tr = eng.get_trajectory(T)
    return tr["logp"].reshape(P, 4), tr["advantages"].reshape(P), tr


def _check_reduction(eng, g, P, tag):
    """(1) the record against the float64 aggregation of terms32 on the kernel's own lp"""
    st, lp, _ = eng.policy_stats(per_sample=True)
    L, adv, _ = _buffer(eng, P)
    assert (g["samples"], g["skipped"]) == (st["samples"], st["skipped"]), tag
    use = statsref.counted(L)
    assert g["samples"] == int(use.sum()) and g["skipped"] == int((~use).sum()), tag
    N = 4 * g["samples"]
    if N == 0:
        assert all(math.isnan(g[k]) for k in ("grad_surrogate", "grad", "z2_mean")), (tag, g)
        return
    _, c = logstdref.consts32(eng.log_std()["log_std"])
    lp = lp.reshape(P, 4)[use]
    w, zz = logstdref.terms32(lp, L[use], adv[use], c)
    term = w.astype(np.float64) * (zz.astype(np.float64) - 1.0)
    d, b = -g["grad_surrogate"] * N - term.sum(), 4 * U23 * np.abs(term).sum()
    lo, hi = logstdref.zz_bracket(lp, c)
    tol = U52 * hi.sum() / N
    print(tag, f"reduction: |d sum term| {abs(d):.3g} / {b:.3g}; z2_mean {g['z2_mean']:.17g} in "
          f"[{lo.mean():.17g}, {hi.mean():.17g}] -+ {tol:.3g}")
    assert abs(d) <= b, (tag, d, b)
    assert lo.mean() - tol <= g["z2_mean"] <= hi.mean() + tol, (tag, g["z2_mean"], lo.mean(), hi.mean())
    assert g["grad"] == g["grad_surrogate"]  # EntropyCoef = 0


def _check_end_to_end(g, name, P, L, adv, tag, keep=None, s=-1.0):
    """(2) against float64 throughout"""
    keep = np.arange(P) if keep is None else keep
    _, tr = statsref.case(name, P)
    m, A = logstdref.mean64(name, P)[keep], tr["actions"].reshape(P, 4)[keep]
    ref, _, term = logstdref.grad64(m, A, L[keep], adv[keep], s)
    if term.size == 0:
        return
    w, zz, lp64 = logstdref.entries64(m, A, L[keep], adv[keep], s)
    tau = 1e-5 * np.abs(lp64).max() + 2e-5
    b = tau * np.mean(np.abs(w) * (np.abs(zz - 1) + 2)) + 4 * tau ** 2 * np.mean(np.abs(w))
    print(tag, f"end to end: grad {g['grad_surrogate']:.9g} ref {ref:.9g} |d| {abs(g['grad_surrogate'] - ref):.3g} / {b:.3g}; "
          f"z2_mean {g['z2_mean']:.9g} ref {zz.mean():.9g}")
    assert abs(g["grad_surrogate"] - ref) <= b, (tag, g, ref, b)
    assert abs(g["z2_mean"] - zz.mean()) <= 2 * tau, tag  # zz moves by 2 tau


@pytest.mark.parametrize("family,name,P", CASES)
def test_log_std_gradient(wk, family, name, P):
    """(1), (2) and (4)'s determinism: two calls return identical bytes"""
    tag = f"{family}/{name}/P={P}"
    eng = _put(wk, family, name, P)
    g = eng.log_std_gradient()
    _check_reduction(eng, g, P, tag)
    L, adv, _ = _buffer(eng, P)
    _check_end_to_end(g, name, P, L, adv, tag)
    assert _gbytes(eng.log_std_gradient()) == _gbytes(g)


SKIP_CASES = [(fam, name, P, pat)
              for fam, name in FAMILIES[:3] for P in (33, statsref.large_p(fam))
              for pat in statsref.SKIP_PATTERNS if statsref.skip_rows(pat, fam, P) is not None]


@pytest.mark.parametrize("family,name,P,pattern", SKIP_CASES)
def test_skip_rule(wk, family, name, P, pattern):
    """(3) logp_old = -200 in one dimension of the pattern's rows: counts exact, the sums those of
    the case without the rows (within (1)'s and (2)'s bounds), and non-finite skipped rows change
    no byte of the record"""
    rows = statsref.skip_rows(pattern, family, P)
    tag = f"{family}/{name}/P={P}/{pattern}"
    _, base = statsref.case(name, P)
    eng = _put(wk, family, name, P, statsref.with_skips(base, rows))
    g = eng.log_std_gradient()
    keep = np.setdiff1d(np.arange(P), rows)
    assert (g["samples"], g["skipped"]) == (P - len(rows), len(rows)), tag
    _check_reduction(eng, g, P, tag)
    L, adv, _ = _buffer(eng, P)
    _check_end_to_end(g, name, P, L, adv, tag, keep)
    if pattern == "all":
        assert g["samples"] == 0 and math.isnan(g["grad"]) and math.isnan(g["z2_mean"])
    for poison in ("nan", "inf"):
        _put(wk, family, name, P, statsref.with_skips(base, rows, poison=poison), eng)
        gp = eng.log_std_gradient()
        _, advp, _ = _buffer(eng, P)
        assert not np.isfinite(advp[rows]).any()
        assert _gbytes(gp) == _gbytes(g), (tag, poison)


@pytest.mark.parametrize("family,name", TWO)
def test_no_side_effects(wk, family, name):
    """(4) rollout, ppo_update, rollout with and without log_std_gradient calls in between:
    weights, Adam, the trajectory with its returns and advantages, log_std() and the next
    rollout bit-identical"""
    n, T = 64, 8
    out = []
    for probe in (False, True):
        eng = tgs._engine(wk, family, name, n, T, Minibatch=128, Epochs=2, RandomizeStart=1)
        eng.rollout(T)
        if probe:
            a, b = eng.log_std_gradient(), eng.log_std_gradient()
            assert _gbytes(a) == _gbytes(b) and a["samples"] + a["skipped"] == n * T
        eng.compute_returns()
        t0 = eng.get_trajectory(T)
        if probe:
            eng.log_std_gradient()
        t1 = eng.get_trajectory(T)
        for k in t0:
            np.testing.assert_array_equal(t0[k].view(np.uint8), t1[k].view(np.uint8), err_msg=k)
        eng.ppo_update(update_index=0)
        if probe:
            eng.log_std_gradient()
        eng.rollout(T)
        out.append((tgs._state(eng), eng.get_trajectory(T), eng.episode_log_count(), _lbytes(eng.log_std()), t0))
    (sa, ta, la, lsa, t0a), (sb, tb, lb, lsb, t0b) = out
    tgs._same_state(sa, sb)
    assert la == lb and lsa == lsb
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
        np.testing.assert_array_equal(t0a[k], t0b[k], err_msg=k)


def _learn_engine(wk, family, name, **cfg):
    return tgs._stop_engine(wk, family, name, SEED, LearnLogStd=1, **cfg)


@pytest.mark.parametrize("coef", [0.0, 0.01])
@pytest.mark.parametrize("family,name", TWO)
def test_step_bit_for_bit(wk, family, name, coef):
    """(5) Alpha = 0 (set_learning_rate: wk_create wants Alpha > 0): no weight moves, so epoch k's
    gradient is what log_std_gradient() returns at s_k, and the update's three steps replay with
    set_log_std + log_std_gradient + logstdref.adam_scalar bit for bit.  64 walkers x 16 steps,
    4 minibatches"""
    cfg = dict(LogStdAlpha=1e-2, EntropyCoef=coef)
    eng = _learn_engine(wk, family, name, **cfg)
    eng.set_learning_rate(0.0)
    eng.rollout(16)
    w0 = eng.get_weights().view(np.uint32).copy()
    s0 = eng.log_std()
    assert _lbytes(s0) == _lbytes(dict(s0, m=0.0, v=0.0, grad_last=0.0, t=0, steps=0, clamped=0, nonfinite=0))
    assert s0["log_std"] == -1.0 and abs(s0["entropy"] - (-1.0 + 0.5 * math.log(2 * math.pi * math.e))) <= 1e-15
    eng.ppo_update(epochs=3, update_index=0)
    np.testing.assert_array_equal(eng.get_weights().view(np.uint32), w0)
    got = eng.log_std()
    # the replay on a second context with the same rollout
    rep = _learn_engine(wk, family, name, **cfg)
    rep.rollout(16)
    np.testing.assert_array_equal(rep.get_weights().view(np.uint32), w0)
    c = rep.cfg
    s, m, v, t = -1.0, 0.0, 0.0, 0
    for k in range(3):
        g = rep.log_std_gradient()
        assert g["grad"] == g["grad_surrogate"] - float(F(coef))
        s, m, v, t, clamped, stepped = logstdref.adam_scalar(
            s, m, v, t, g["grad"], float(F(1e-2)), float(c.Beta1), float(c.Beta2), float(c.AdamEpsilon),
            float(c.LogStdMin), float(c.LogStdMax))
        assert stepped and not clamped
        rep.set_log_std(s)
        print(f"{family}/{name} coef {coef} epoch {k}: grad {g['grad']:.9g} z2_mean {g['z2_mean']:.6g} -> s {s:.9g}")
    want = dict(rep.log_std(), m=m, v=v, t=t, grad_last=g["grad"], steps=3, clamped=0, nonfinite=0)
    assert _lbytes(got) == _lbytes(want), (got, want)
    assert got["steps"] == 3 and got["t"] == 3 and got["log_std"] != -1.0
    assert got["std"] == float(logstdref.consts32(got["log_std"])[0])
    if coef > 0:  # the bonus pushes s up: a lower gradient than without
        assert g["grad"] < g["grad_surrogate"]


def _tight_engine(wk, family, name, P, negated, **cfg):
    w, traj = logstdref.tight(name, P, negated=negated)
    eng = _put(wk, family, name, P, traj, weights=w, LearnLogStd=1, Minibatch=16, Epochs=1, **cfg)
    eng.set_learning_rate(0.0)
    return eng


@pytest.mark.parametrize("family,name", TWO)
def test_direction(wk, family, name):
    """(9) actions closer to the mean than std says, positive advantages: log_std falls and the
    gradient is positive; with negated advantages it rises"""
    for negated in (False, True):
        eng = _tight_engine(wk, family, name, 33, negated, LogStdAlpha=1e-2)
        z2 = eng.log_std_gradient()["z2_mean"]
        eng.ppo_update(update_index=0)
        s = eng.log_std()
        print(f"{family}/{name} negated={negated}: z2_mean {z2:.4g} grad_last {s['grad_last']:.6g} log_std {s['log_std']:.9g}")
        assert z2 < 0.3 and s["steps"] == 1 and s["t"] == 1
        if negated:
            assert s["grad_last"] < 0 and s["log_std"] > -1.0
        else:
            assert s["grad_last"] > 0 and s["log_std"] < -1.0
        assert abs(abs(s["log_std"] + 1.0) - 1e-2) < 1e-6  # Adam's first step is lr sign(g)


def test_clamp_and_nonfinite(wk):
    """(6) the clamp: LogStdMax one float above the start, a step of about +1 lands exactly on it
    and is counted.  Non-finite: a NaN advantage in a counted row takes no step in any epoch"""
    hi = float(np.nextafter(F(-1.0), F(0)))
    eng = _tight_engine(wk, "builtin", "default", 33, True, LogStdAlpha=1.0, LogStdMax=hi)
    eng.ppo_update(update_index=0)
    s = eng.log_std()
    assert (s["log_std"], s["steps"], s["clamped"], s["nonfinite"], s["t"]) == (hi, 1, 1, 0, 1), s
    assert s["std"] == float(logstdref.consts32(hi)[0])
    # a NaN reward makes the row's return and advantage NaN; logp_old keeps the row counted
    w, traj = logstdref.tight("default", 33)
    bad = {k: v.copy() for k, v in traj.items()}
    bad["rewards"].reshape(-1)[5] = np.nan
    eng = _put(wk, "builtin", "default", 33, bad, weights=w, LearnLogStd=1, Minibatch=16, Epochs=3, LogStdAlpha=1e-2)
    eng.set_log_std_adam(0.25, 0.5, 7)
    before = eng.log_std()
    g = eng.log_std_gradient()
    assert g["samples"] == 33 and math.isnan(g["grad"])
    eng.ppo_update(update_index=0)
    s = eng.log_std()
    assert (s["nonfinite"], s["steps"], s["clamped"]) == (3, 0, 0) and math.isnan(s["grad_last"])
    assert _lbytes(s, ("m", "v", "t")) == _lbytes(before, ("m", "v", "t")) and (s["m"], s["v"], s["t"]) == (0.25, 0.5, 7)


@pytest.mark.parametrize("family,name", TWO)
def test_pinned(wk, family, name):
    """(7) LogStdMin == LogStdMax == LogStandardDeviation: the log-std cannot move, so a 5-epoch
    update leaves weights and Adam bit-equal to a LearnLogStd = 0 context's, and with TargetKL
    halfway between two epochs' KLs it stops at the same epoch with a byte-equal record (the one
    pass per epoch serves both)"""
    pin = dict(LogStdMin=-1.0, LogStdMax=-1.0)
    for seed in range(SEED, SEED + 5):  # test_gpu_stats.test_early_stop's choice of seed and epoch
        runs = tgs._epoch_runs(family, name, seed)
        kls = [r[0] for r in runs]
        ks = [k for k in range(2, 5) if kls[k - 1] > max(kls[:k - 1])]
        if ks:
            break
    assert ks, kls
    k = ks[0]
    eng = tgs._stop_engine(wk, family, name, seed, LearnLogStd=1, **pin)
    eng.rollout(16)
    eng.ppo_update(update_index=0)
    tgs._same_state(tgs._state(eng), runs[4][1])
    s = eng.log_std()
    assert (s["log_std"], s["steps"], s["t"], s["nonfinite"]) == (-1.0, 5, 5, 0)
    assert _lbytes(s, ()) == _lbytes(tgs._stop_engine(wk, family, name, seed).log_std(), ())  # the create-time bits
    with pytest.raises(wk.WkError):
        eng.update_stats()  # TargetKL = 0: no check was recorded
    target = float(F((kls[k - 1] + max(kls[:k - 1])) / 2))
    recs = []
    for cfg in (dict(), dict(LearnLogStd=1, **pin)):
        e = tgs._stop_engine(wk, family, name, seed, TargetKL=target, **cfg)
        e.rollout(16)
        e.ppo_update(update_index=0)
        us = e.update_stats()
        assert (us["epochs_run"], us["stopped_early"]) == (k, 1)
        tgs._same_state(tgs._state(e), runs[k - 1][1])
        recs.append(tgs._bytes(us))
    assert recs[0] == recs[1]
    assert e.log_std()["steps"] == k  # pass, log-std step, stop decision


@pytest.mark.parametrize("family,name", TWO)
def test_new_std_everywhere(wk, family, name):
    """(8) after set_log_std(-0.3) on an otherwise default context every kernel uses the new std"""
    n, T, s_new = 64, 8, -0.3
    c, a = netref.NETS[name]
    old = tgs._engine(wk, family, name, n, T, RandomizeStart=1)
    eng = tgs._engine(wk, family, name, n, T, RandomizeStart=1)
    eng.set_log_std(s_new)
    st = eng.log_std()
    std_new, _ = logstdref.consts32(s_new)
    assert st["log_std"] == float(F(s_new)) and st["std"] == float(std_new) and (st["t"], st["m"], st["v"]) == (0, 0.0, 0.0)
    wa = eng.get_weights()[netref.n_params(c):]
    rng = np.random.default_rng(11)
    obs = rng.normal(0, 1, (40, 12)).astype(F)
    ids, steps = np.arange(40, dtype=np.int32) * 3, np.arange(40, dtype=np.uint32) + 5
    m0, a0, _ = old.policy_sample(obs, ids, steps)
    m1, a1, lp1 = eng.policy_sample(obs, ids, steps)
    np.testing.assert_array_equal(m0.view(np.uint32), m1.view(np.uint32))
    # act = mean + std z with the same z: act - mean scales by the ratio of the fp32 stds.  Both
    # differences carry the rounding of act (half a place of |act| <= |mean| + |d|) and of the
    # product std z, on either side of the comparison: 4 * 2^-23 relative to |mean| + |d|
    ratio = float(std_new) / float(logstdref.consts32(-1.0)[0])
    d0, d1 = (a0 - m0).astype(np.float64) * ratio, (a1 - m1).astype(np.float64)
    assert (np.abs(d1 - d0) <= 4 * U23 * (np.abs(m1) + np.abs(d0))).all()
    assert np.abs(d1).max() > 1.5 * np.abs(a0 - m0).max()  # (it did move)
    _, lp64 = netref.policy64(a, wa, obs, a1, log_std=s_new)
    np.testing.assert_allclose(lp1, lp64, rtol=1e-5, atol=2e-5)
    ss = eng.step_sampled(2)
    _, lp64 = netref.policy64(a, wa, ss["states"].reshape(-1, 12), ss["actions"].reshape(-1, 4), log_std=s_new)
    np.testing.assert_allclose(ss["logp"].reshape(-1, 4), lp64, rtol=1e-5, atol=2e-5)
    # the rollout records log-densities under the new std and the statistics pass reproduces them
    eng.rollout(T)
    lp = eng.get_trajectory(T)["logp"]
    ps = eng.policy_stats()
    delta = 2 * (1e-5 * np.abs(lp).max() + 2e-5)
    print(f"{family}/{name}: ratio_max {ps['ratio_max']:.9g} kl {ps['kl']:.3g}, delta {delta:.3g}")
    assert ps["samples"] > 0 and ps["ratio_max"] <= math.exp(delta) and 0 <= ps["kl"] <= math.expm1(delta) - delta
    _, lp64 = netref.policy64(a, wa, eng.get_trajectory(T)["states"].reshape(-1, 12),
                              eng.get_trajectory(T)["actions"].reshape(-1, 4), log_std=s_new)
    np.testing.assert_allclose(lp.reshape(-1, 4), lp64, rtol=1e-5, atol=2e-5)
    # back to the create-time value: the create-time bits
    eng2 = tgs._engine(wk, family, name, n, T, RandomizeStart=1)
    eng2.set_log_std(s_new)
    eng2.set_log_std(-1.0)
    assert _lbytes(eng2.log_std()) == _lbytes(old.log_std())
    eng2.rollout(T)
    old.rollout(T)
    ta, tb = eng2.get_trajectory(T), old.get_trajectory(T)
    for k in ta:
        np.testing.assert_array_equal(ta[k].view(np.uint8), tb[k].view(np.uint8), err_msg=k)


def _version(path):
    with open(path, "rb") as f:
        return struct.unpack("<I", f.read(8)[4:])[0]


@pytest.mark.parametrize("family,name", TWO)
def test_lifecycle(wk, family, name, tmp_path):
    """(10) snapshot and checkpoint carry the log-std and its Adam state"""
    cfg = dict(LogStdAlpha=1e-2, EntropyCoef=0.01)
    eng = _learn_engine(wk, family, name, **cfg)
    eng.rollout(16)
    eng.ppo_update(update_index=0)
    s1 = eng.log_std()
    assert s1["steps"] == 5 and s1["log_std"] != -1.0
    # snapshot save / update / restore
    eng.snapshot()
    eng.ppo_update(update_index=7)
    assert _lbytes(eng.log_std()) != _lbytes(s1)
    eng.restore()
    assert _lbytes(eng.log_std()) == _lbytes(s1)
    # checkpoint round trip into a fresh context, then the same next iteration
    ck = str(tmp_path / "ls.ckpt")
    eng.checkpoint_save(ck)
    assert _version(ck) == 6
    fresh = _learn_engine(wk, family, name, **cfg)
    fresh.checkpoint_load(ck)
    keys = ("m", "v", "entropy", "t")
    assert _lbytes(fresh.log_std(), keys) == _lbytes(s1, keys)
    for e in (eng, fresh):
        e.rollout(16)
        e.ppo_update(update_index=1)
    tgs._same_state(tgs._state(eng), tgs._state(fresh))
    assert _lbytes(eng.log_std()) == _lbytes(fresh.log_std()) and eng.log_std()["t"] == 10
    # a LearnLogStd = 0 context: version 4 / 5, whatever set_log_std was called with
    plain, moved = (tgs._stop_engine(wk, family, name, SEED) for _ in range(2))
    moved.set_log_std(-0.3)
    pa, pb = str(tmp_path / "plain.ckpt"), str(tmp_path / "moved.ckpt")
    plain.checkpoint_save(pa)
    moved.checkpoint_save(pb)
    assert _version(pa) == _version(pb) == (4 if family == "builtin" else 5)
    with open(pa, "rb") as fa, open(pb, "rb") as fb:
        ba, bb = fa.read(), fb.read()
    assert len(ba) == len(bb) and ba == bb
    with open(ck, "rb") as f:
        assert len(f.read()) == len(ba) + 24
    moved.checkpoint_load(pa)
    assert moved.log_std()["log_std"] == float(F(-0.3))  # configuration: not checkpointed
    # loading across LearnLogStd is an error either way, and leaves the contexts working
    for e, p in ((plain, ck), (fresh, pa)):
        with pytest.raises(wk.WkError) as ex:
            e.checkpoint_load(p)
        assert "(-1)" in str(ex.value) and "LearnLogStd" in str(ex.value)  # WK_ERR_ARG
    assert _lbytes(fresh.log_std()) == _lbytes(eng.log_std())


def test_refusals(wk):
    """(11)"""
    lib = wk.load_library()

    def refused(**cfg):
        with pytest.raises(wk.WkError) as ex:
            wk.Engine(8, seed=SEED, Horizon=4, **cfg)
        assert "(-3)" in str(ex.value), (cfg, str(ex.value))  # WK_ERR_CONFIG
        msg = lib.wk_last_error(None).decode()
        assert msg and msg in str(ex.value)
        return msg

    nan, inf = float("nan"), float("inf")
    for v in (2, -1):
        assert "LearnLogStd" in refused(LearnLogStd=v)
    for v in (-1e-3, nan, inf):
        assert "LogStdAlpha" in refused(LogStdAlpha=v)
        assert "LogStdAlpha" in refused(LearnLogStd=1, LogStdAlpha=v)
        assert "EntropyCoef" in refused(LearnLogStd=1, EntropyCoef=v)
    assert "EntropyCoef" in refused(EntropyCoef=0.01)  # a constant with a fixed std
    for kw in (dict(LogStdMin=-5.0), dict(LogStdMin=-0.5), dict(LogStdMax=-1.5), dict(LogStdMax=5.0),
               dict(LogStdMin=nan), dict(LogStdMax=nan), dict(LogStdMin=-6.0, LogStdMax=6.0)):
        assert "LogStdMin" in refused(LearnLogStd=1, **kw)
    # ... and unchecked with LearnLogStd = 0
    plain = wk.Engine(8, seed=SEED, Horizon=4, LogStdMin=3.0, LogStdMax=-3.0)
    learn = wk.Engine(8, seed=SEED, Horizon=4, LearnLogStd=1, LogStdMin=-2.0, LogStdMax=0.0)

    def arg_error(f, *a, code="(-1)"):  # WK_ERR_ARG
        before = _lbytes(f.__self__.log_std())
        with pytest.raises(wk.WkError) as ex:
            f(*a)
        assert code in str(ex.value), str(ex.value)
        assert _lbytes(f.__self__.log_std()) == before

    for e in (plain, learn):
        for v in (nan, inf, -inf, 5.0, -5.0, 7.0):
            arg_error(e.set_log_std, v)
    for v in (-2.5, 0.5):
        arg_error(learn.set_log_std, v)
    plain.set_log_std(4.5)
    learn.set_log_std(-2.0)
    learn.set_log_std(0.0)
    arg_error(plain.set_log_std_adam, 0.0, 0.0, 0, code="(-5)")  # WK_ERR_STATE
    for a in ((nan, 0.0, 0), (0.0, inf, 0), (0.0, -1.0, 0), (0.0, 0.0, -1), (inf, 0.0, 0)):
        arg_error(learn.set_log_std_adam, *a)
    learn.set_log_std_adam(-0.5, 2.0, 3)
    s = learn.log_std()
    assert (s["m"], s["v"], s["t"], s["log_std"]) == (-0.5, 2.0, 3, 0.0)
    p = plain.log_std()
    assert (p["t"], p["m"], p["v"], p["steps"], p["clamped"], p["nonfinite"], p["grad_last"]) == (0, 0.0, 0.0, 0, 0, 0, 0.0)
    assert p["log_std"] == 4.5 and abs(p["entropy"] - (4.5 + 0.5 * math.log(2 * math.pi * math.e))) <= 1e-15
    # one GPU
    with pytest.raises(wk.WkError) as ex:
        learn.comm_init_host(0, 1, lambda buf: None)
    assert "(-3)" in str(ex.value) and "LearnLogStd" in str(ex.value)
    with pytest.raises(wk.WkError) as ex:
        learn.comm_ipc_handle()
    assert "(-3)" in str(ex.value)
    # no trajectory yet
    for e in (plain, learn):
        with pytest.raises(wk.WkError) as ex:
            e.log_std_gradient()
        assert "(-5)" in str(ex.value)
    # still working contexts
    learn.set_log_std(-1.0)
    learn.rollout(4)
    g = learn.log_std_gradient()
    assert g["samples"] + g["skipped"] == 32
