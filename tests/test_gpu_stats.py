"""GPU: wk_policy_stats / wk_update_stats_get and the TargetKL early stop, on the built-in kernels
(k_ppo_stats) and the general ones (k_net_stats) -- tests/statsref.py holds the cases and the
float64 restatement, tests/test_statsref.py the conditions the exact counts rest on.

Every case goes through set_trajectory + set_weights + policy_stats(per_sample=True).
  (a) per-row log-densities and values against float64 at the project's bar for trajectory
      log-probabilities and values (rtol 1e-5, atol 2e-5; tests/test_gpu_net.py::test_rollout);
  (b) the reduction alone: every statistic against a float64 aggregation of the kernel's own
      per-row outputs and the buffer's fp32 inputs.  Counts exact; a mean of N terms that never
      pass through expf within 2^-52 sum|term| (the sum within N 2^-52 sum|term|, divided by N);
      the surrogate within 4 * 2^-23 of sum|term| / N and ratio_max within 4 * 2^-23 relative
      (device and numpy expf may differ in the last place); explained variance within 1e-9;
  (c) end to end against float64 with bounds propagated from (a), first order plus the square:
      tau = 1e-5 max|lp64| + 2e-5, tau_v the same on the values.
P: 1, 15, 16, 17, 33 and per family one row past a whole grid pass (statsref.large_p: 32,769 for
the built-in kernel, 16,385 = 145 * 113 for the general one).  Every case prints its figures
(pytest -s)."""
import functools

import numpy as np
import pytest

import netref
import statsref

pytestmark = pytest.mark.gpu

SEED = 20250905
F = np.float32
U52, U23 = 2.0 ** -52, 2.0 ** -23
FLOATS = ("kl", "kl_k1", "clip_fraction", "ratio_max", "surrogate", "value_loss", "explained_variance")
FAMILIES = [("builtin", "default"), ("general", "default"), ("general", "odd"), ("general", "edge16")]
CASES = [(fam, name, P) for fam, name in FAMILIES for P in statsref.SMALL_P + (statsref.large_p(fam),)]


def _engine(wk, family, name, n, T, **cfg):
    if family == "builtin":
        return wk.Engine(n, seed=SEED, Horizon=T, **cfg)
    c, a = netref.NETS[name]
    return wk.Engine(n, seed=SEED, Horizon=T, NetworkKernels=1, CriticNeuralNetwork=c,
                     ActorNeuralNetwork=a, **cfg)


def _run(wk, family, name, P, traj=None, eng=None):
    """(stats dict, lp_new [P, 4], v_new [P], the buffer's fp32 logp_old, returns, advantages, engine)"""
    w, base = statsref.case(name, P)
    traj = base if traj is None else traj
    n, T = statsref.SHAPES[P]
    if eng is None:
        eng = _engine(wk, family, name, n, T)
    eng.set_weights(w)
    eng.set_trajectory(**traj)
    st, lp, v = eng.policy_stats(per_sample=True)
    tr = eng.get_trajectory(T)
    return st, lp.reshape(P, 4), v.reshape(P), tr["logp"].reshape(P, 4), tr["returns"].reshape(P), \
        tr["advantages"].reshape(P), eng


def _bytes(st):
    """a record's bytes (NaN-safe equality)"""
    return [int(st[k]) for k in ("samples", "skipped", "epochs_run", "stopped_early")] + \
        [np.float64(st[k]).tobytes() for k in FLOATS]


def _close(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def _check_reduction(st, lp, v, L, ret, adv, tag):
    """(b): the record against the float64 aggregation of the kernel's own per-row outputs"""
    use = statsref.counted(L)
    ref = statsref.stats64(lp, v, L, ret, adv, fp32_diff=True)
    N = 4 * ref["samples"]
    assert (st["samples"], st["skipped"]) == (ref["samples"], ref["skipped"]), tag
    assert st["epochs_run"] == 0 and st["stopped_early"] == 0
    if N == 0:
        assert all(np.isnan(st[k]) for k in FLOATS), (tag, st)
        return ref
    # the fp32 ratios and surrogate terms, as the kernel forms them
    with np.errstate(over="ignore"):
        r32 = np.exp((lp[use] - L[use]).astype(F))
    lo, up = F(1) - F(statsref.EPS_CLIP), F(1) + F(statsref.EPS_CLIP)
    a32 = adv[use][:, None].astype(F)
    sur = np.minimum(r32 * a32, np.clip(r32, lo, up) * a32).astype(np.float64)
    clipped = int(((r32 > up) | (r32 < lo)).sum())
    fig = dict(kl=(st["kl"] - ref["kl"], U52 * ref["abs"]["kl"]),
               kl_k1=(st["kl_k1"] - ref["kl_k1"], U52 * ref["abs"]["kl_k1"]),
               value_loss=(st["value_loss"] - ref["value_loss"], U52 * ref["abs"]["value_loss"]),
               surrogate=(st["surrogate"] - sur.mean(), 4 * U23 * np.abs(sur).sum() / N),
               ratio_max=(st["ratio_max"] - float(r32.max()), 4 * U23 * float(r32.max())))
    print(tag, "reduction:", {k: f"{abs(d):.3g} / {b:.3g}" for k, (d, b) in fig.items()})
    assert st["clip_fraction"] == clipped / N and clipped == ref["clipped"], tag
    for k, (d, b) in fig.items():
        assert abs(d) <= b, (tag, k, d, b)
    assert _close(st["explained_variance"], ref["explained_variance"], 1e-9), (tag, st, ref)
    return ref


def _check_end_to_end(st, name, P, L, ret, adv, tag, keep=None):
    """(c): against float64 throughout, with the per-row bar propagated"""
    lp64, V64 = statsref.forward64(name, P)
    keep = np.arange(P) if keep is None else keep
    ref = statsref.stats64(lp64[keep], V64[keep], L[keep], ret[keep], adv[keep])
    if ref["samples"] == 0:
        return
    tau = 1e-5 * np.abs(lp64[keep]).max() + 2e-5
    tau_v = 1e-5 * np.abs(V64[keep]).max() + 2e-5
    fig = dict(kl=(st["kl"] - ref["kl"], tau * np.abs(np.expm1(ref["d"])).mean() + tau ** 2),
               kl_k1=(st["kl_k1"] - ref["kl_k1"], tau),
               value_loss=(st["value_loss"] - ref["value_loss"], 2 * tau_v * np.abs(ref["e"]).mean() + tau_v ** 2))
    print(tag, "end to end:", {k: f"{abs(d):.3g} / {b:.3g}" for k, (d, b) in fig.items()})
    for k, (d, b) in fig.items():
        assert abs(d) <= b, (tag, k, d, b)
    assert st["clip_fraction"] == ref["clip_fraction"], tag  # every ratio 1e-3 from a bound


@pytest.mark.parametrize("family,name,P", CASES)
def test_policy_stats(wk, family, name, P):
    tag = f"{family}/{name}/P={P}"
    st, lp, v, L, ret, adv, eng = _run(wk, family, name, P)
    lp64, V64 = statsref.forward64(name, P)
    np.testing.assert_allclose(lp, lp64, rtol=1e-5, atol=2e-5)  # (a)
    np.testing.assert_allclose(v, V64, rtol=1e-5, atol=2e-5)
    _check_reduction(st, lp, v, L, ret, adv, tag)  # (b)
    _check_end_to_end(st, name, P, L, ret, adv, tag)  # (c)
    if P == 1:
        assert np.isnan(st["explained_variance"])  # one row has no variance
    # (e) two calls return identical bytes
    st2, lp2, v2 = eng.policy_stats(per_sample=True)
    assert _bytes(st2) == _bytes(st)
    np.testing.assert_array_equal(lp2.reshape(P, 4).view(np.uint32), lp.view(np.uint32))
    np.testing.assert_array_equal(v2.reshape(P).view(np.uint32), v.view(np.uint32))
    assert _bytes(eng.policy_stats()) == _bytes(st)  # without the per-row outputs


# `default` (both families) and `odd` at P = 33 and the large P, every pattern that exists there (the
# built-in kernel's 33 rows are one block's: no second block)
SKIP_CASES = [(fam, name, P, pat)
              for fam, name in FAMILIES[:3] for P in (33, statsref.large_p(fam))
              for pat in statsref.SKIP_PATTERNS if statsref.skip_rows(pat, fam, P) is not None]


@pytest.mark.parametrize("family,name,P,pattern", SKIP_CASES)
def test_skip_rule(wk, family, name, P, pattern):
    """(d) logp_old = -200 in one dimension of the pattern's rows"""
    rows = statsref.skip_rows(pattern, family, P)
    tag = f"{family}/{name}/P={P}/{pattern}"
    _, base = statsref.case(name, P)
    st, lp, v, L, ret, adv, eng = _run(wk, family, name, P, statsref.with_skips(base, rows))
    keep = np.setdiff1d(np.arange(P), rows)
    assert (st["samples"], st["skipped"]) == (P - len(rows), len(rows)), tag
    lp64, V64 = statsref.forward64(name, P)
    np.testing.assert_allclose(lp, lp64, rtol=1e-5, atol=2e-5)  # every row, the skipped too
    np.testing.assert_allclose(v, V64, rtol=1e-5, atol=2e-5)
    _check_reduction(st, lp, v, L, ret, adv, tag)
    _check_end_to_end(st, name, P, L, ret, adv, tag, keep)
    if pattern == "all":
        assert st["samples"] == 0 and all(np.isnan(st[k]) for k in FLOATS)
    # non-finite skipped rows change no byte of the record.  The buffer's returns and advantages
    # come from its rewards and old values, so they are poisoned together: NaN rewards make both
    # NaN, -inf rewards make both -inf
    for poison in ("nan", "inf"):
        sp, lpp, vp, _, retp, advp, _ = _run(wk, family, name, P, statsref.with_skips(base, rows, poison=poison), eng)
        assert not np.isfinite(retp[rows]).any() and not np.isfinite(advp[rows]).any()
        assert (np.isneginf(advp[rows]).all() if poison == "inf" else np.isnan(retp[rows]).all())
        assert _bytes(sp) == _bytes(st), (tag, poison)
        np.testing.assert_array_equal(lpp[keep].view(np.uint32), lp[keep].view(np.uint32))


@pytest.mark.parametrize("family,name", [("builtin", "default"), ("general", "odd")])
def test_small_call_after_large_equals_fresh_context(wk, family, name):
    """(e) the scratch's old contents are never read: the P = 17 case after the large P on one
    context (one walker, so that both sizes are horizons of the same context) equals a fresh
    context's"""
    P = statsref.large_p(family)

    def put(eng, q):
        w, traj = statsref.case(name, q)
        eng.set_weights(w)
        eng.set_trajectory(**{k: v.reshape((q, 1) + v.shape[2:]) for k, v in traj.items()})

    eng = _engine(wk, family, name, 1, P)
    put(eng, P)
    assert eng.policy_stats()["samples"] == P
    put(eng, 17)
    a = eng.policy_stats(per_sample=True)
    fresh = _engine(wk, family, name, 1, P)
    put(fresh, 17)
    b = fresh.policy_stats(per_sample=True)
    assert a[0]["samples"] == 17 and _bytes(a[0]) == _bytes(b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    # the same rows as 17 walkers of one step each: the same record
    assert _bytes(_run(wk, family, name, 17)[0]) == _bytes(a[0])


def _state(eng):
    m, v, t = eng.get_adam()
    return eng.get_weights().view(np.uint32), m.view(np.uint32), v.view(np.uint32), t


@pytest.mark.parametrize("family,name", [("builtin", "default"), ("general", "odd")])
def test_no_side_effects(wk, family, name):
    """(f) rollout, ppo_update, rollout with and without policy_stats calls in between: weights,
    Adam and the next rollout's actions bit-identical, the logs as long"""
    n, T = 64, 8
    out = []
    for probe in (False, True):
        eng = _engine(wk, family, name, n, T, Minibatch=128, Epochs=2, RandomizeStart=1)
        eng.rollout(T)
        if probe:
            s = eng.policy_stats()
            # the collecting policy itself: d is the rollout's and this pass's rounding of one
            # log-density, within the bar tau of (a), and expm1(d) - d <= tau^2 for |d| <= tau < 1
            tau = 1e-5 * np.abs(eng.get_trajectory(T)["logp"]).max() + 2e-5
            assert s["samples"] + s["skipped"] == n * T and 0 <= s["kl"] <= tau ** 2 and abs(s["kl_k1"]) <= tau
            eng.policy_stats(per_sample=True)
        eng.ppo_update(update_index=0)
        if probe:
            assert eng.policy_stats()["kl"] > 0
        eng.rollout(T)
        out.append((_state(eng), eng.get_trajectory(T), eng.episode_log_count()))
    (sa, ta, la), (sb, tb, lb) = out
    for x, y in zip(sa[:3], sb[:3]):
        np.testing.assert_array_equal(x, y)
    assert sa[3] == sb[3] and la == lb
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)


@functools.lru_cache(maxsize=None)
def _epoch_runs(family, name, seed):
    """fresh TargetKL = 0 contexts with epochs = 1..5 on the same seed's rollout:
    [(kl after the update, weights / Adam state)]"""
    import wk
    runs = []
    for k in range(1, 6):
        eng = _stop_engine(wk, family, name, seed)
        eng.rollout(16)
        eng.ppo_update(epochs=k, update_index=0)
        runs.append((eng.policy_stats()["kl"], _state(eng)))
    return runs


def _stop_engine(wk, family, name, seed, **cfg):
    kw = dict(Horizon=16, Minibatch=256, Epochs=5, RandomizeStart=1, **cfg)
    if family == "builtin":
        return wk.Engine(64, seed=seed, **kw)
    c, a = netref.NETS[name]
    return wk.Engine(64, seed=seed, NetworkKernels=1, CriticNeuralNetwork=c, ActorNeuralNetwork=a, **kw)


def _same_state(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3]


@pytest.mark.parametrize("family,name", [("builtin", "default"), ("general", "odd")])
def test_early_stop(wk, family, name):
    """(g) 64 walkers, Horizon 16, minibatch 256: four minibatches per epoch"""
    # the first of at most five seeds with some k < 5 whose kl exceeds every earlier epoch's
    for seed in range(SEED, SEED + 5):
        runs = _epoch_runs(family, name, seed)
        kls = [r[0] for r in runs]
        ks = [k for k in range(2, 5) if kls[k - 1] > max(kls[:k - 1])]
        if ks:
            break
    print(f"{family}/{name}: seed {seed}, kl after epochs 1..5: {kls}")
    assert ks, kls
    k = ks[0]
    assert runs[4][1][3] == 20  # Adam's step count: 5 epochs of 4 minibatches
    # TargetKL = 0: no check was made
    eng = _stop_engine(wk, family, name, seed)
    eng.rollout(16)
    eng.ppo_update(update_index=0)
    with pytest.raises(wk.WkError) as ex:
        eng.update_stats()
    assert "(-5)" in str(ex.value)  # WK_ERR_STATE
    _same_state(_state(eng), runs[4][1])
    # a target never reached: five epochs, five checks, the same bits as without
    eng = _stop_engine(wk, family, name, seed, TargetKL=1e9)
    with pytest.raises(wk.WkError):
        eng.update_stats()  # no update yet
    eng.rollout(16)
    eng.ppo_update(update_index=0)
    us = eng.update_stats()
    assert (us["epochs_run"], us["stopped_early"]) == (5, 0)
    _same_state(_state(eng), runs[4][1])
    assert np.float64(us["kl"]).tobytes() == np.float64(kls[4]).tobytes()
    # halfway between kl_k and the largest earlier one: stops after exactly k epochs
    target = float(F((kls[k - 1] + max(kls[:k - 1])) / 2))
    assert max(kls[:k - 1]) < target < kls[k - 1]
    eng = _stop_engine(wk, family, name, seed, TargetKL=target)
    eng.rollout(16)
    cd, ad = eng.ppo_update(update_index=0)
    us = eng.update_stats()
    assert (us["epochs_run"], us["stopped_early"]) == (k, 1)
    st = _state(eng)
    assert st[3] == 4 * k
    _same_state(st, runs[k - 1][1])
    assert np.float64(us["kl"]).tobytes() == np.float64(kls[k - 1]).tobytes()
    assert np.isfinite([cd, ad]).all()
    # any movement at all passes 1e-30: one epoch
    eng = _stop_engine(wk, family, name, seed, TargetKL=1e-30)
    eng.rollout(16)
    eng.ppo_update(update_index=0)
    us = eng.update_stats()
    assert (us["epochs_run"], us["stopped_early"]) == (1, 1) and eng.get_adam()[2] == 4
    _same_state(_state(eng), runs[0][1])


def test_refusals(wk):
    """(h)"""
    eng = wk.Engine(8, seed=SEED, Horizon=4, TargetKL=0.01)
    with pytest.raises(wk.WkError) as ex:
        eng.comm_init_host(0, 1, lambda buf: None)
    assert "(-3)" in str(ex.value) and "TargetKL" in str(ex.value)  # WK_ERR_CONFIG
    with pytest.raises(wk.WkError) as ex:
        eng.comm_ipc_handle()
    assert "(-3)" in str(ex.value)
    with pytest.raises(wk.WkError) as ex:
        eng.comm_init(0, 1, bytes(128))
    assert "(-3)" in str(ex.value)
    with pytest.raises(wk.WkError) as ex:
        eng.comm_init_ipc_records(0, 1, [bytes(wk.IPC_HANDLE_BYTES)])
    assert "(-3)" in str(ex.value)
    for e in (eng, wk.Engine(8, seed=SEED, Horizon=4)):
        with pytest.raises(wk.WkError) as ex:
            e.policy_stats()  # no trajectory yet
        assert "(-5)" in str(ex.value)  # WK_ERR_STATE
    # ReturnsMode 1 without bootstrap values: wk_ppo_update's rule
    w, traj = statsref.case("default", 16)
    e1 = wk.Engine(4, seed=SEED, Horizon=4, ReturnsMode=1)
    e1.set_trajectory(**traj)
    with pytest.raises(wk.WkError, match="bootstrap"):
        e1.policy_stats()
    e1.set_bootstrap_values(np.zeros(4, F))
    assert e1.policy_stats()["samples"] == 16
    # a still-working context after the refusals
    eng.rollout(4)
    assert eng.policy_stats()["samples"] + eng.policy_stats()["skipped"] == 32
