"""CPU: the general numpy restatement used by the general networks' GPU tests (tests/netref.py)
agrees, for the default strings, with the float64 restatement of the built-in network
(tests/ref64.py) and with the oracle's fp32 forward pass."""
import numpy as np
import pytest

import net_cases
import netref
import ref64

F = np.float32
CD, AD = netref.CRITIC_DEFAULT, netref.ACTOR_DEFAULT


def test_layers():
    assert netref.layers(AD) == [("D", 12, 64), ("LeakyReLU", 64, 64), ("D", 64, 64),
                                 ("LeakyReLU", 64, 64), ("D", 64, 4), ("TanH", 4, 4)]
    assert netref.layers(netref.NETS["odd"][1])[:3] == [("TanH", 12, 12), ("D", 12, 7), ("ReLU", 7, 7)]
    assert netref.n_params(CD) + netref.n_params(AD) == ref64.NPARAM
    assert sum(netref.n_params(s) for s in netref.NETS["max"]) == 70021


def test_grad64_equals_ref64_on_the_golden_batch(golden):
    g = golden("train_batch.npz")
    args = (g["w0"], g["states"], g["actions"], g["logp_old"], g["returns"], g["adv"], 64)
    a = netref.train_batch_grad64(CD, AD, *args)
    b = ref64.train_batch_grad64(*args)
    scale = np.abs(b[0]).max()
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * scale
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(b[1]).max()
    assert a[2] == pytest.approx(b[2], rel=1e-12) and a[3] == pytest.approx(b[3], rel=1e-12)
    assert a[4] == b[4]


def test_grad64_skip_rule_equals_ref64():
    rng = np.random.default_rng(5)
    B = 33
    w = rng.normal(0, 0.2, ref64.NPARAM).astype(F)
    S, A = rng.normal(0, 1, (B, 12)).astype(F), rng.normal(0, 1, (B, 4)).astype(F)
    L = rng.normal(-3, 1, (B, 4)).astype(F)
    L[7, 3] = -200.0
    G, Ad = rng.normal(0, 5, B).astype(F), rng.normal(0, 1, B).astype(F)
    a = netref.train_batch_grad64(CD, AD, w, S, A, L, G, Ad, B)
    b = ref64.train_batch_grad64(w, S, A, L, G, Ad, B)
    assert a[4] == b[4] == 1
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(b[0]).max()


def test_forward32_matches_the_oracle(orc):
    ag = orc.Agent(seed=20250905)
    w = ag.params()
    S = np.random.default_rng(1).normal(0, 1, (32, 12)).astype(F)
    mean = netref.forward32(AD, w[897:], S)
    val = netref.forward32(CD, w[:897], S)
    for i in range(len(S)):
        np.testing.assert_allclose(mean[i], ag.mean(S[i]), rtol=1e-6, atol=1e-6)
        assert abs(val[i, 0] - ag.value(S[i])) <= 1e-6 * (1 + abs(val[i, 0]))


def test_adam32_matches_the_oracle(orc, golden):
    g = golden("train_batch.npz")
    w1, m, v = netref.adam32(g["w0"], np.zeros_like(g["w0"]), np.zeros_like(g["w0"]), g["grads"], 1)
    np.testing.assert_allclose(w1, g["w1"], rtol=0, atol=1e-7)


def test_derivative_at_zero_is_one():
    z = np.zeros(3, F)
    assert (netref._dact("ReLU", z) == 1).all() and (netref._dact("LeakyReLU", z) == 1).all()


# ---- the inputs of tests/test_gpu_net_edges.py (tests/net_cases.py) ----
def test_edge_networks_parse_within_the_limits():
    for name in netref.EDGE_NAMES:
        for dsl, out in zip(netref.NETS[name], (1, 4)):
            L = netref.layers(dsl)
            dense = [l for l in L if l[0] == "D"]
            assert len(L) <= 8 and 1 <= len(dense) <= 4 and dense[-1][2] == out
            assert max(o for _, _, o in dense) <= 128
    assert netref.NETS["big_critic"] == (netref.NETS["max"][0], netref.NETS["tiny"][1])
    assert netref.NETS["big_actor"] == (netref.NETS["tiny"][0], netref.NETS["max"][1])


def test_grad32_is_the_same_code_in_fp32():
    w, batch = net_cases.draw("odd", 33, 1033)
    c, a = netref.NETS["odd"]
    g32 = netref.train_batch_grad32(c, a, w, *batch, 33)
    g64 = netref.train_batch_grad64(c, a, w, *batch, 33)
    assert g32[0].dtype == g32[1].dtype == F and g64[0].dtype == np.float64
    assert type(g32[2]) is F and type(g32[3]) is F
    assert 0 < np.abs(g32[0] - g64[0]).max() <= 1e-5 * np.abs(g64[0]).max()
    assert g32[4] == g64[4] == 0


def test_case_table_is_complete():
    assert set(net_cases.CASES) == {(n, B) for n in netref.EDGE_NAMES for B in net_cases.BS}
    assert len(net_cases.CASES) == 56 and not net_cases.NO_SEED
    assert not set(net_cases.CASES) & set(net_cases.EXTRA_CASES)


@pytest.mark.parametrize("name", netref.EDGE_NAMES + ["extra"])
def test_case_seeds_keep_the_restatement_within_half_the_bound(name):
    """the condition that keeps the GPU test from blaming a kernel for a ReLU / LeakyReLU branch
    flip: on every case's inputs the fp32 restatement is within half the bound and the seed is one
    of the five candidates (`python tests/net_cases.py` prints what the earlier ones gave).

    The restatement's own rounding follows the CPU's BLAS and SIMD kernels (matrix products,
    exp, tanh).  With OpenBLAS's AVX-512 kernel sets the worst case is 0.387 (`edge16`, B = 17),
    with its AVX2 sets (Haswell, Zen) 0.433 (`edge64`, B = 17); with the FMA-less Sandybridge set
    `edge128` at B = 16385 rounds into a branch flip (0.72): a miss here on such a machine says
    that about the machine's fp32, not about a kernel."""
    table = net_cases.EXTRA_CASES if name == "extra" else \
        {k: v for k, v in net_cases.CASES.items() if k[0] == name}
    assert table
    for (net, B), seed in table.items():
        k, rem = divmod(seed - (1000 + B), 100)
        assert rem == 0 and 0 <= k < net_cases.MAX_SEEDS, (net, B, seed)
        w, batch = net_cases.draw(net, B, seed)
        assert not (np.exp(batch[2]) == 0).any()  # no skipped sample
        ratio = net_cases.restatement_ratio(net, w, batch)
        print(f"net {net:10s} B {B:6d} seed {seed:6d}  fp32 restatement / bound = {ratio:.3f}")
        assert ratio <= net_cases.HALF, (net, B, seed, ratio)


@pytest.mark.parametrize("B", [33, 16385])
@pytest.mark.parametrize("name", ["odd", "edge16"])
def test_skip_patterns_of_the_reference(name, B):
    """the reference drops exactly the marked rows, and the restatement stays within half the
    bound but for the one recorded exception (net_cases.SKIP_ABOVE_HALF)"""
    w, base = net_cases.case(name, B)
    c, a = netref.NETS[name]
    for pattern in net_cases.SKIP_PATTERNS:
        rows = net_cases.skip_rows(pattern, B)
        if rows is None:
            continue
        batch = net_cases.with_skips(base, rows)
        g64, asum, cd, ad, sk = netref.train_batch_grad64(c, a, w, *batch, B)
        assert sk == len(rows)
        if pattern == "all":
            assert not g64.any() and not asum.any() and cd == 0 and ad == 0
            continue
        assert np.isfinite(g64).all() and np.abs(g64).max() > 0
        ratio = net_cases.restatement_ratio(name, w, batch)
        print(f"net {name:8s} B {B:6d} skip {pattern:7s}  fp32 restatement / bound = {ratio:.3f}")
        known = net_cases.SKIP_ABOVE_HALF.get((name, B, pattern))
        if known is None:
            assert ratio <= net_cases.HALF, (name, B, pattern, ratio)
        else:  # recorded, not chosen: the inputs are fixed by the table's case
            assert ratio > net_cases.HALF, "the record is out of date"
    assert net_cases.skip_rows("block1", 16385)[0] == 32 and net_cases.skip_rows("block1", 33) is None


@pytest.mark.parametrize("name", sorted(net_cases.SURROGATE_CASES))
def test_surrogate_batch_populates_the_six_cells(name):
    seed = net_cases.SURROGATE_CASES[name]
    k, rem = divmod(seed - 2000, 100)
    assert rem == 0 and 0 <= k < net_cases.MAX_SEEDS
    w, batch = net_cases.surrogate_draw(name, seed)
    S, A, L, G, Ad = batch
    r, counts, loss_sum = net_cases.surrogate_cells(name, w, batch)
    print(f"net {name}: cells [Adv < 0, Adv > 0] x [r < 0.7, inside, r > 1.3] = {counts.tolist()}")
    assert counts.shape == (2, 3) and counts.sum() == 4 * net_cases.SURROGATE_B
    assert (counts >= 8).all(), counts
    for edge in (0.7, 1.3):  # fp32 and float64 on the same side of the clip edges
        assert (np.abs(r - edge) >= 1e-3 * edge).all()
    assert (np.abs(Ad) >= 0.1).all() and (Ad > 0).any() and (Ad < 0).any()
    ratio = net_cases.restatement_ratio(name, w, batch)
    print(f"net {name}: fp32 restatement / bound = {ratio:.3f}")
    assert ratio <= net_cases.HALF
    # the per-cell statement of the loss derivative is the reference's: the bias gradient of a
    # last dense layer with no activation behind it is the per-dimension sum of actorLoss
    if name == "odd":
        c, a = netref.NETS[name]
        g64 = netref.train_batch_grad64(c, a, w, *batch, len(G))[0]
        np.testing.assert_allclose(g64[-4:], loss_sum, rtol=1e-12, atol=0)


# ---- the inputs of tests/test_gpu_grad_edges.py (the built-in matrix-core kernels) ----
# sha256 over the bytes of (weights, S, A, L, G, Ad) of the B = 96 draws, taken from surrogate_draw
# as it was before it took keywords (fixed B = 96, log-std -1, RHO)
B96_SHA256 = {
    "odd": "1b8b56b13459013dd07ff5ec557ad2483bfd514069ec49d9091ad1c6fc9da2e8",
    "default": "4e332a8135d94a4eb3cd04ee39f99f32318f814a392308101f3b1fd1c0793bb3",
}


def test_generalised_surrogate_draw_keeps_the_b96_batch():
    """the keywords' defaults reproduce the B = 96 draws byte for byte (actions and logp_old pass
    through a float64 forward pass on their way to fp32: a BLAS whose float64 sums differ in the
    last bit moves an fp32 rounding with a probability near 1e-8 per entry)"""
    import hashlib
    assert set(B96_SHA256) == set(net_cases.SURROGATE_CASES)
    for name, seed in net_cases.SURROGATE_CASES.items():
        w, batch = net_cases.surrogate_draw(name, seed)
        assert len(batch[3]) == net_cases.SURROGATE_B == 96
        h = hashlib.sha256()
        for x in (w, *batch):
            h.update(x.tobytes())
        assert h.hexdigest() == B96_SHA256[name], name


def test_grad_edge_table_is_complete():
    want = {(B, "default") for B in net_cases.GRAD_EDGE_BS} | {(B, "tight") for B in net_cases.TIGHT_BS}
    assert set(net_cases.GRAD_EDGE_CASES) == want and len(want) == 17


@pytest.mark.parametrize("B,variant", sorted(net_cases.GRAD_EDGE_CASES))
def test_grad_edge_case_meets_its_conditions(B, variant):
    """the seed is one of the five candidates 2000 + B, + 100, ..., no sample is skipped, the fp32
    restatement stays within half the bar, the ratios keep clear of the clip edges (fp32 and
    float64 on the same side) and, from B = 96 and on every non-default case, each of the six cells
    sign(Adv) x {r < 1 - eps, inside, r > 1 + eps} holds at least B // 12 entries (the cycle gives
    B / 2, B and B / 2 per sign)"""
    seed = net_cases.GRAD_EDGE_CASES[(B, variant)]
    k, rem = divmod(seed - (2000 + B), 100)
    assert rem == 0 and 0 <= k < net_cases.MAX_SEEDS
    _, ref_kw = net_cases.grad_edge_params(variant)
    w, batch = net_cases.grad_edge_case(B, variant)
    assert len(batch[3]) == B and not (np.exp(batch[2]) == 0).any()
    ratio = net_cases.restatement_ratio("default", w, batch, **ref_kw)
    r, counts, _ = net_cases.surrogate_cells("default", w, batch, **ref_kw)
    print(f"B {B:6d} {variant:8s} seed {seed:6d}  fp32 restatement / bound = {ratio:.3f}  cells {counts.tolist()}")
    assert ratio <= net_cases.HALF, (B, variant, seed, ratio)
    eps = ref_kw.get("eps_clip", 0.3)
    for edge in (1.0 - eps, 1.0 + eps):
        assert (np.abs(r - edge) >= 1e-3 * edge).all()
    assert counts.sum() == 4 * B
    if B >= 96 or variant != "default":
        assert (counts >= B // 12).all(), counts
    assert (np.abs(batch[4]) >= 0.1).all()


def test_ref64_equals_netref_on_the_surrogate_batch():
    w, batch = net_cases.surrogate_case("default")
    a = netref.train_batch_grad64(CD, AD, w, *batch, 96)
    b = ref64.train_batch_grad64(w, *batch, 96)
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(b[0]).max()
    assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(b[1]).max()
    assert a[2] == pytest.approx(b[2], rel=1e-12) and a[3] == pytest.approx(b[3], rel=1e-12) and a[4] == b[4] == 0
    kw = dict(log_std=-0.5, eps_clip=0.1)
    w, batch = net_cases.grad_edge_case(96, "tight")
    a = netref.train_batch_grad64(CD, AD, w, *batch, 96, **kw)
    b = ref64.train_batch_grad64(w, *batch, 96, **kw)
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(b[0]).max()


def test_sweep_positions():
    B, P = net_cases.SWEEP_B, net_cases.SWEEP_POSITIONS
    assert B == 16 * 1024 + 7 and len(set(P)) == len(P) == 27 and max(P) == B - 1
    assert set(range(16)) <= set(P) and {16, 32, 48, 64} <= set(P)
    for units in (256, 512, 1024):  # tp<1>, tp<2>, ws / mfma: last unit of a pass, first of the next
        assert 16 * (units - 1) in P and 16 * units in P
    w, batch = net_cases.surrogate_draw("default", net_cases.SWEEP_SEED, B=B)
    one = tuple(x[:1] for x in batch)  # the live row: a non-zero gradient in both networks
    g64 = netref.train_batch_grad64(CD, AD, w, *one, B)[0]
    assert g64[:897].any() and g64[897:].any()


@pytest.mark.parametrize("shape", sorted(net_cases.PERM_CASES))
def test_perm_cases_meet_their_conditions(orc, shape):
    """every minibatch of the keyed permutation is without repeats (over the whole epoch too), and
    the float64 gradient of each has non-zero actor and critic entries (so Adam's moments, which the
    GPU test compares bit for bit, see every minibatch)"""
    from conftest import SEED
    n, T, M, E = shape
    pool, nmb = n * T, (n * T) // M
    assert nmb >= 1 and nmb * M <= pool
    w, traj = net_cases.perm_trajectory(shape)
    ret, adv = np.empty((T, n), F), np.empty((T, n), F)
    for i in range(n):
        ret[:, i], adv[:, i] = orc.returns_mc(traj["rewards"][:, i], traj["values"][:, i], traj["dones"][:, i], 0.9)
    assert (adv > 0).any() and (adv < 0).any()
    rows = (traj["states"].reshape(pool, 12), traj["actions"].reshape(pool, 4), traj["logp"].reshape(pool, 4),
            ret.reshape(pool), adv.reshape(pool))
    for e in range(E):
        idx_all = orc.perm_batch(nmb * M, pool, orc.perm_key(SEED, net_cases.PERM_UPDATE, e))
        assert len(np.unique(idx_all)) == len(idx_all) and idx_all.max() < pool
        assert not np.array_equal(idx_all, np.arange(len(idx_all)))
        for j in range(nmb):
            idx = idx_all[j * M:(j + 1) * M]
            g64, _, _, _, sk = ref64.train_batch_grad64(w, *(x[idx] for x in rows), M)
            assert sk == 0 and g64[:897].any() and g64[897:].any()
