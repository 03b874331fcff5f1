"""GPU: the general networks' kernels (NetworkKernels = 1, csrc/wk_net.hip) and their host loop
(net_sampled, csrc/wk_api_env.cpp) where tests/test_gpu_net.py does not reach:

  * widths next to the tile edges (netref.NETS edge16 .. edge128: 15 / 16 / 17, 31 / 32 / 33,
    63 / 64 / 65, 127 / 128 against `out` per 16 and `in` per 4, 16 and 32), widths 1 to 3
    (`narrow`), activations stacked on the input and on each other (`stacked`), and the pairs in
    which the critic alone or the actor alone sets the rows of the activation cache (`big_*`);
  * the tile-to-block assignment around B = 16384 / 16385 (one tile per block -> two, the last
    block with one live sample), the reduction groups at 16 / 17 blocks, and a slab buffer that
    an earlier, larger call has filled;
  * the skip rule on a full tile's first sample, a whole tile, the first sample of a later block,
    every sample, and with non-finite values in the skipped rows;
  * all six cells sign(Adv) x {r < 1 - eps, inside, r > 1 + eps} of the clipped surrogate at
    ratios near 1, as in training;
  * Adam's m and v bit for bit and the weight step within a derived bound;
  * rollouts across episode ends (MaxTimesteps = 5), a reset(mask) and a second rollout, MC and
    GAE returns across `done`, NormalizeAdvantages, and the episode / loss logs.

Inputs: tests/net_cases.py.  Every gradient case's seed was chosen on the CPU by the reference
alone so that a plain fp32 numpy evaluation of the same math stays within half the bar
(tests/test_netref.py re-checks it without a GPU); the GPU decides nothing about its inputs, and
a GPU ratio above 1.0 is a finding about the kernel.  One exception is recorded there:
the whole-tile skip on `edge16` at B = 33, whose inputs are fixed (the table's B = 33 case with
rows 16..31 dropped) and on which the fp32 restatement itself is at 1.51 of the bar (the kernel:
0.325).

Bars: the gradient bar |g - g64| <= 1e-5 * sum|t| + 1e-7 * max|g64| and the diagnostics' 1e-5 *
(|x| + 1) of tests/test_gpu_net.py; rtol = atol = 1e-5 for the forward pass; atol 1e-6 for the
noise; bit equality for physics, returns, logs, Adam's moments and every repeat; for the weights
after Adam |dw| <= ulp(w) + 4 * 2^-23 * |step| (one rounding of the subtraction, at most one ulp
on each of the four operations that form the step).  The float64 reference of every gradient case
takes well under a second, so every network runs every B.  Each case prints its worst ratio
(pytest -s; measured values: DESIGN.md "General networks").
"""
import functools

import numpy as np
import pytest

import net_cases
import netref
from test_gpu_data import Book, _as_tuples
from test_gpu_net import LP_CONST, SEED, STD, _engine, _forward, _weights

pytestmark = pytest.mark.gpu

F = np.float32


@functools.lru_cache(maxsize=None)
def _ref(name, B):
    """(weights, batch, float64 reference) of a table case, computed once; read-only"""
    w, batch = net_cases.case(name, B)
    c, a = netref.NETS[name]
    ref = netref.train_batch_grad64(c, a, w, *batch, B)
    for x in (w, *batch, ref[0], ref[1]):
        x.setflags(write=False)
    return w, batch, ref


def _check(tag, got, ref):
    """the project's gradient bar and the diagnostics' bar; prints the worst ratio"""
    g, cd, ad, sk = got
    g64, asum, cd64, ad64, sk64 = ref
    assert np.isfinite(g).all()
    err, bound = np.abs(g - g64), 1e-5 * asum + 1e-7 * np.abs(g64).max()
    ratio = err / np.where(bound > 0, bound, 1.0)  # (every sample skipped: the bound is 0)
    worst = int(np.argmax(ratio))
    print(f"{tag}  np {g.size:6d}  worst |g - g64| / bound = {ratio[worst]:.3f} (param {worst})")
    assert (err <= bound).all(), (tag, worst, float(ratio[worst]))
    assert sk == sk64
    assert abs(cd - cd64) <= 1e-5 * (abs(cd64) + 1.0) and abs(ad - ad64) <= 1e-5 * (abs(ad64) + 1.0)


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _same_bits(a, b):
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
    assert _bits([a[1], a[2]]).tolist() == _bits([b[1], b[2]]).tolist() and a[3] == b[3]


# ---- 1. every table case against float64 ----
@pytest.mark.parametrize("B", net_cases.BS)
@pytest.mark.parametrize("name", netref.EDGE_NAMES)
def test_gradient_edge_case_vs_f64(wk, name, B):
    w, batch, ref = _ref(name, B)
    eng = _engine(wk, name)
    eng.set_weights(w)
    got = eng.minibatch_gradient(*batch)
    assert got[3] == 0
    _check(f"net {name:10s} B {B:6d}", got, ref)


# ---- 2. forward pass ----
@pytest.mark.parametrize("n", [1, 15, 16, 17])
@pytest.mark.parametrize("name", netref.EDGE_NAMES)
def test_forward_edge_networks(wk, name, n):
    S = np.random.default_rng(n).normal(0, 1, (n, 12)).astype(F)
    w = _weights(name)
    eng = _engine(wk, name)
    eng.set_weights(w)
    mean, act, lp = eng.policy_sample(S)
    val = eng.value(S)
    rmean, rval = _forward(name, w, S)
    np.testing.assert_allclose(mean, rmean, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(val, rval, rtol=1e-5, atol=1e-5)
    ref_lp = LP_CONST - ((act.astype(np.float64) - mean) / STD) ** 2 / 2
    np.testing.assert_allclose(lp, ref_lp, rtol=1e-5, atol=1e-5)


# ---- 3. the slab buffer after a larger call ----
def test_stale_slab_changes_nothing(wk):
    """B = 16385 leaves 513 slabs behind (the read-modify-write path of the second tile of each
    block); B = 17 then uses two of them, and must not see what they hold"""
    w, big, _ = _ref("edge16", 16385)
    w17, small, ref17 = _ref("edge16", 17)
    eng = _engine(wk, "edge16")
    eng.set_weights(w)
    first = eng.minibatch_gradient(*big)
    eng.set_weights(w17)
    mid = eng.minibatch_gradient(*small)
    eng.set_weights(w)
    third = eng.minibatch_gradient(*big)
    _same_bits(first, third)
    fresh = _engine(wk, "edge16")
    fresh.set_weights(w17)
    _same_bits(mid, fresh.minibatch_gradient(*small))
    _check("net edge16 after B 16385: B 17", mid, ref17)


# ---- 4. reduction group edges ----
@pytest.mark.parametrize("B", [256, 257])
def test_reduction_group_edges(wk, B):
    """16 tiles = 16 blocks = one full group of RG = 16; 17 blocks = a second group of one"""
    w, batch, ref = _ref("narrow", B)
    eng = _engine(wk, "narrow")
    eng.set_weights(w)
    _check(f"net narrow     B {B:6d}", eng.minibatch_gradient(*batch), ref)


# ---- 5. the skip rule ----
SKIPS = [(name, B, p) for name in ("odd", "edge16") for B in (33, 16385) for p in net_cases.SKIP_PATTERNS
         if net_cases.skip_rows(p, B) is not None]


@pytest.mark.parametrize("name,B,pattern", SKIPS)
def test_skip_patterns(wk, name, B, pattern):
    """rows with logp_old[i, 2] = -200 (exp == 0 in fp32): the reference `continue`s before it
    touches such a sample; the kernel computes on and selects zeros, so what the skipped rows
    hold otherwise -- here NaN states and returns, +inf actions, -inf advantages -- must change
    no bit.  (`edge16` at B = 33 with the whole tile dropped: the fp32 restatement itself is at
    1.51 of the bar on these inputs, tests/net_cases.py SKIP_ABOVE_HALF.)"""
    w, base, _ = _ref(name, B)
    c, a = netref.NETS[name]
    rows = net_cases.skip_rows(pattern, B)
    batch = net_cases.with_skips(base, rows)
    ref = netref.train_batch_grad64(c, a, w, *batch, B)
    assert ref[4] == len(rows)
    eng = _engine(wk, name)
    eng.set_weights(w)
    got = eng.minibatch_gradient(*batch)
    assert got[3] == ref[4]
    _check(f"net {name:10s} B {B:6d} skip {pattern:6s}", got, ref)
    if pattern == "all":
        assert not got[0].any() and got[1] == 0.0 and got[2] == 0.0
        return
    _same_bits(got, eng.minibatch_gradient(*net_cases.with_skips(base, rows, poison=True)))


# ---- 6. the six cells of the clipped surrogate ----
@pytest.mark.parametrize("name", sorted(net_cases.SURROGATE_CASES))
def test_surrogate_cells(wk, name):
    w, batch = net_cases.surrogate_case(name)
    c, a = netref.NETS[name]
    B = net_cases.SURROGATE_B
    r, counts, loss_sum = net_cases.surrogate_cells(name, w, batch)
    assert (counts >= 8).all(), counts  # (and the other input conditions: tests/test_netref.py)
    ref = netref.train_batch_grad64(c, a, w, *batch, B)
    eng = _engine(wk, name)
    eng.set_weights(w)
    got = eng.minibatch_gradient(*batch)
    _check(f"net {name:10s} B {B:6d} six cells", got, ref)
    if name == "odd":
        # no activation behind the last dense layer: its bias gradient is the per-dimension sum
        # of actorLoss, here against the sum written out cell by cell
        bound = 1e-5 * ref[1][-4:] + 1e-7 * np.abs(ref[0]).max()
        err = np.abs(got[0][-4:] - loss_sum)
        print(f"net odd six cells: last bias gradient, worst |g - sum| / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), (err, bound)


# ---- 7. Adam in k_net_reduce ----
@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("name", ["odd", "edge128"])
def test_adam_moments_bit_exact(wk, name, t0):
    """m and v are products and sums only and the build has contraction off: bit equality with
    netref.adam32 fed the gradient the call returned.  The weights: w - alpha * mhat / (sqrt(vhat)
    + eps), compared within one rounding of the subtraction plus one ulp on each of the division
    by the bias corrections (two), the square root and the quotient."""
    w, batch, _ = _ref(name, 33)
    eng = _engine(wk, name)
    eng.set_weights(w)
    m0, v0 = net_cases.adam_state(eng.nparam, 40 + t0)
    assert (m0 != 0).all() and (v0 >= 0).all() and v0.any()
    eng.set_adam(m0, v0, t0)
    g, _, _, _ = eng.train_batch(*batch, apply_adam=True)
    rw, rm, rv = netref.adam32(w, m0, v0, g, t0 + 1)
    m, v, t = eng.get_adam()
    assert t == t0 + 1
    np.testing.assert_array_equal(_bits(m), _bits(rm))
    np.testing.assert_array_equal(_bits(v), _bits(rv))
    gw = eng.get_weights()
    mh = rm.astype(np.float64) / float(F(1.0 - float(F(0.9)) ** t))
    vh = rv.astype(np.float64) / float(F(1.0 - float(F(0.999)) ** t))
    step = float(F(1e-3)) * mh / (np.sqrt(vh) + float(F(1e-8)))
    bound = np.spacing(np.abs(rw)).astype(np.float64) + 4 * 2.0 ** -23 * np.abs(step)
    diff = np.abs(gw.astype(np.float64) - rw)
    unequal = int((_bits(gw) != _bits(rw)).sum())
    print(f"net {name:10s} Adam t {t0:3d} -> {t:4d}: {unequal} of {gw.size} weights not bit-equal, "
          f"worst |dw| / bound = {(diff / bound).max():.3f}")
    assert (diff <= bound).all(), (int(np.argmax(diff / bound)), float((diff / bound).max()))
    assert (gw != w).any()


# ---- 8. rollouts across episode ends ----
def _replay(orc, envs, tr, tag):
    """the oracle replays the recorded actions: states, rewards and dones bit for bit"""
    T, n = tr["rewards"].shape
    for i, e in enumerate(envs):
        for t in range(T):
            np.testing.assert_array_equal(tr["states"][t, i], e.obs(), err_msg=f"{tag} env {i} t {t}")
            _, r, d = e.step(tr["actions"][t, i])
            assert r == tr["rewards"][t, i] and d == tr["dones"][t, i], (tag, i, t)


def _noise(eng, tr):
    mean, _, _ = eng.policy_sample(tr["states"].reshape(-1, 12))
    return tr["actions"].reshape(-1, 4) - mean


@pytest.mark.parametrize("name,n,lanes,rough", [
    ("odd", 64, 1, 0), ("odd", 64, 2, 0), ("odd", 64, 4, 0), ("odd", 17, 1, 0), ("edge16", 64, 2, 1),
    ("default", 1, 1, 0)])
def test_rollout_across_episode_ends(wk, orc, name, n, lanes, rough):
    T = 24
    cfg = dict(Horizon=T, MaxTimesteps=5, RandomizeStart=1, LanesPerWalker=lanes, RoughFloor=rough)
    eng = _engine(wk, name, n=n, **cfg)
    w = orc.Agent(seed=SEED).params() if name == "default" else _weights(name, 3)
    eng.set_weights(w)
    base = wk.Engine(n, seed=SEED, **cfg)  # the built-in kernels, their own weights
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    trs, btrs = [], []
    for k in range(2):
        for e, out in ((eng, trs), (base, btrs)):
            e.rollout(T)
            out.append(e.get_trajectory(T))
            if k == 0:
                e.reset(mask)
    envs = [orc.Env(dx=float(orc.env_offset(SEED, i)), rough=(SEED, i) if rough else None, MaxTimesteps=5)
            for i in range(n)]
    for k, tr in enumerate(trs):
        assert (tr["dones"].sum(axis=0) >= 3).all(), tr["dones"].sum(axis=0).min()
        _replay(orc, envs, tr, f"rollout {k}")
        if k == 0:
            for i in np.nonzero(mask)[0]:
                envs[i].reset()
        for i in range(n):
            ret, adv = orc.returns_mc(tr["rewards"][:, i], tr["values"][:, i], tr["dones"][:, i], 0.9)
            np.testing.assert_array_equal(ret, tr["returns"][:, i])
            np.testing.assert_array_equal(adv, tr["advantages"][:, i])
        S = tr["states"].reshape(n * T, 12)
        rmean, rval = _forward(name, w, S)
        np.testing.assert_allclose(tr["values"].reshape(-1), rval, rtol=1e-5, atol=1e-5)
        ref_lp = LP_CONST - ((tr["actions"].reshape(-1, 4).astype(np.float64) - rmean) / STD) ** 2 / 2
        np.testing.assert_allclose(tr["logp"].reshape(-1, 4), ref_lp, rtol=1e-5, atol=2e-5)
        # the noise depends on the global walker id and the step counter alone: the built-in
        # context, driven through the same calls, pins the counter across episode ends, the reset
        # and the second rollout
        noise = _noise(eng, tr)
        assert np.abs(noise).max() > 0.05
        np.testing.assert_allclose(noise, _noise(base, btrs[k]), rtol=0, atol=1e-6, err_msg=f"rollout {k}")
    # the second rollout continued the first: the unmasked walkers' first states are where the
    # first rollout left them (the oracle replay above), the masked ones start from the template
    assert not np.array_equal(trs[0]["actions"], trs[1]["actions"])


def test_gae_and_normalize_across_episode_ends(wk, orc):
    n, T = 16, 16
    eng = _engine(wk, "odd", n=n, Horizon=T, MaxTimesteps=5, UseGAE=1, NormalizeAdvantages=1)
    eng.set_weights(_weights("odd", 3))
    eng.rollout(T)
    tr = eng.get_trajectory(T)
    assert (tr["dones"].sum(axis=0) >= 2).all()  # (an episode of MaxTimesteps = 5 has 6 steps)
    adv = np.zeros((T, n), F)
    for i in range(n):
        ret, a = orc.returns_gae(tr["rewards"][:, i], tr["values"][:, i], tr["dones"][:, i], 0.9, 0.95)
        np.testing.assert_array_equal(tr["returns"][:, i], ret)
        adv[:, i] = a
    np.testing.assert_allclose(tr["advantages"], orc.normalize(adv.reshape(-1), 0.3).reshape(T, n),
                               rtol=1e-5, atol=1e-6)


def test_episode_and_loss_logs(wk):
    n, T = 256, 32
    eng = _engine(wk, "tiny", n=n, Horizon=T, MaxTimesteps=10, Minibatch=512, Epochs=1)
    book = Book(n)
    expect, diags = [], []
    for k in range(3):
        eng.rollout(T)
        tr = eng.get_trajectory(T)
        expect += book.rollout(tr["rewards"], tr["dones"])
        diags.append(eng.ppo_update(update_index=k))
        if k == 1:
            mask = (np.arange(n) % 3 == 0).astype(np.uint8)
            eng.reset(mask)
            book.reset(mask.astype(bool))
    recs, dropped = eng.drain_episodes()
    got = _as_tuples(recs)
    assert dropped == 0 and len(got) == len(expect) >= 3 * 2 * n  # (11-step episodes, 32-step rollouts)
    for g, x in zip(got, expect):
        assert g[1:] == tuple(int(v) for v in x[1:]) and _bits(g[0]) == _bits(x[0]), (g, x)
    cl, al = eng.drain_losses()
    np.testing.assert_array_equal(_bits(cl), _bits([d[0] for d in diags]))
    np.testing.assert_array_equal(_bits(al), _bits([d[1] for d in diags]))
    assert eng.drain_episodes()[0].size == 0
