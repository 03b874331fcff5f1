"""GPU parity of the benchmarked PPO gradient path at full size (VERDICT r1 items 1 / ADVICE).

`wk_ppo_update` runs `k_ppo_grad_mfma` with the grid capped at 256 blocks x 4 waves, so
above 16,384 samples every wave loops over several 16-sample chunks (next-chunk gather
prefetch, accumulators carried across chunks).  These tests drive exactly that path through
the C ABI (`wk_minibatch_gradient`, the same kernel and reduction) and compare it with the
oracle's sequential `Train(Batch)` (PPOAgent.cs:218-346):

  * B = 65,536 -- the bench's per-GPU minibatch (4 chunks per wave);
  * B = 20,011 -- above 16,384, not a multiple of 16 (ragged last chunk), with one sample
    whose exp(logp_old) underflows to 0 (HadamardDivision throws -> skipped, still / B);
  * one whole `wk_ppo_update` at BASELINE config 3's shape (4,096 walkers, M = 4,096,
    keyed Feistel minibatches) against the oracle running the same minibatch sequence.

Tolerance.  At B = 65,536 the reference's own sequential fp32 sum is the least accurate of
the three: against the float64 restatement of the same math (tests/ref64.py) the oracle is
off by up to 1.3e-4 (scale 0.65; 1.5e-4 of sum|t| where the terms share a sign) -- the sequential sum's own rounding -- while the GPU's
blocked sums (16-sample MFMA blocks, 1,024 wave partials in a fixed tree) stay closer.
So each parameter p is checked against float64:
  |g_gpu[p] - g64[p]| <= 1e-5 * sum_i |t_i[p]| + 1e-7 * max|g64|   (fp32 blocked summation)
the GPU must be no less accurate than the oracle (max error), and GPU vs oracle may differ by
the oracle's own error plus that bound.  Same skip bookkeeping and diagnostics.
"""
import numpy as np
import pytest

import ref64

pytestmark = pytest.mark.gpu

SEED = 20250905
F = np.float32


def _batch(B, seed, skip_at=None):
    rng = np.random.default_rng(seed)
    S = rng.normal(0, 1, (B, 12)).astype(F)
    A = rng.normal(0, 1, (B, 4)).astype(F)
    L = rng.normal(-3, 1, (B, 4)).astype(F)
    G = rng.normal(0, 5, B).astype(F)
    Ad = rng.normal(0, 1, B).astype(F)
    if skip_at is not None:
        L[skip_at, 2] = -200.0  # exp(logp_old) == 0 in fp32: the sample is skipped
    return S, A, L, G, Ad


@pytest.mark.parametrize("B,skip_at", [(65536, None), (65536, 40000), (20011, 5), (20011, 20010)])
def test_minibatch_gradient_multichunk_vs_oracle(wk, orc, B, skip_at):
    ag = orc.Agent(seed=SEED)
    eng = wk.Engine(4, seed=SEED)
    eng.set_weights(ag.params())
    S, A, L, G, Ad = _batch(B, B + (skip_at or 0), skip_at)
    g, cd, ad, sk = eng.minibatch_gradient(S, A, L, G, Ad)
    og, ocd, oad, osk = ag.train_batch(S, A, L, G, Ad, b_div=B, apply_adam=False)
    g64, asum, cd64, ad64, sk64 = ref64.train_batch_grad64(ag.params(), S, A, L, G, Ad, B)
    _check_against_f64(g, og, g64, asum)
    assert sk == osk == sk64 == (0 if skip_at is None else 1)
    assert abs(cd - cd64) <= 1e-5 * (abs(cd64) + 1.0) and abs(ad - ad64) <= 1e-5 * (abs(ad64) + 1.0)
    assert cd == pytest.approx(ocd, rel=2e-4, abs=1e-6) and ad == pytest.approx(oad, rel=2e-4, abs=1e-6)


@pytest.mark.parametrize("impl", ["ws", "tp", "tp1", "mf"])
@pytest.mark.parametrize("B,skip_at", [(8192, 77), (20011, 20010), (600, None), (17, 16), (1, None)])
def test_every_gradient_kernel_vs_f64(wk, orc, monkeypatch, impl, B, skip_at):
    """each matrix-core kernel (WK_GRAD_IMPL, read at wk_create): producer / consumer pairs,
    tile-parallel teams (two or one per block, the default below 32,768 samples) and one wave
    per chunk; 8,192 = one chunk per team (the 8-GPU shard's minibatch), 20,011 = several chunks
    per team with a ragged last chunk, 600 = fewer chunks than teams"""
    monkeypatch.setenv("WK_GRAD_IMPL", impl)
    ag = orc.Agent(seed=SEED)
    eng = wk.Engine(4, seed=SEED)
    eng.set_weights(ag.params())
    S, A, L, G, Ad = _batch(B, B + 7 * (skip_at or 0), skip_at)
    g, cd, ad, sk = eng.minibatch_gradient(S, A, L, G, Ad)
    og, ocd, oad, osk = ag.train_batch(S, A, L, G, Ad, b_div=B, apply_adam=False)
    g64, asum, cd64, ad64, sk64 = ref64.train_batch_grad64(ag.params(), S, A, L, G, Ad, B)
    _check_against_f64(g, og, g64, asum)
    assert sk == osk == sk64 == (0 if skip_at is None else 1)
    assert abs(cd - cd64) <= 1e-5 * (abs(cd64) + 1.0) and abs(ad - ad64) <= 1e-5 * (abs(ad64) + 1.0)


@pytest.mark.parametrize("B", [3856, 4096])
def test_reduction_group_edges_vs_f64(wk, orc, B):
    """the one-launch ordered reduction (the only one) at its group edges, under the default kernel
    choice (tp1: one 16-sample chunk per block): 3,856 samples = 241 slabs, 15 full groups of 16
    and a group of one; 4,096 = 256 slabs, the cap of every gradient launch"""
    ag = orc.Agent(seed=SEED)
    eng = wk.Engine(4, seed=SEED)
    assert eng.grad_kernel(B) == "k_ppo_grad_tp1"
    eng.set_weights(ag.params())
    S, A, L, G, Ad = _batch(B, B)
    g, cd, ad, sk = eng.minibatch_gradient(S, A, L, G, Ad)
    og, ocd, oad, osk = ag.train_batch(S, A, L, G, Ad, b_div=B, apply_adam=False)
    g64, asum, cd64, ad64, sk64 = ref64.train_batch_grad64(ag.params(), S, A, L, G, Ad, B)
    _check_against_f64(g, og, g64, asum)
    assert sk == osk == sk64 == 0
    assert abs(cd - cd64) <= 1e-5 * (abs(cd64) + 1.0) and abs(ad - ad64) <= 1e-5 * (abs(ad64) + 1.0)


def _check_against_f64(g, og, g64, asum):
    assert np.isfinite(g).all()
    scale = np.abs(g64).max()
    e_gpu, e_orc = np.abs(g - g64), np.abs(og - g64)
    bound = 1e-5 * asum + 1e-7 * scale
    worst = int(np.argmax(e_gpu / bound))
    assert (e_gpu <= bound).all(), (
        f"param {worst}: |gpu - f64| = {e_gpu[worst]:.3g} > {bound[worst]:.3g} "
        f"(sum|t| {asum[worst]:.3g}); oracle error there {e_orc[worst]:.3g}")
    assert e_gpu.max() <= e_orc.max() + 1e-7 * scale, (e_gpu.max(), e_orc.max())
    assert (np.abs(g - og) <= e_orc + bound).all()


def test_minibatch_gradient_chunk_split_invariance(wk):
    """Size-independent property of the multi-chunk loop: the gradient of the
    concatenation [X; Y] equals grad(X) * |X|/B + grad(Y) * |Y|/B up to fp32
    re-association (the accumulation across chunks and blocks is a plain sum)."""
    eng = wk.Engine(4, seed=SEED)
    B1, B2 = 24576, 40960
    X = _batch(B1, 1)
    Y = _batch(B2, 2)
    XY = [np.concatenate([x, y]) for x, y in zip(X, Y)]
    B = B1 + B2
    gxy, _, _, _ = eng.minibatch_gradient(*XY, b_div=B)
    gx, _, _, _ = eng.minibatch_gradient(*X, b_div=B)
    gy, _, _, _ = eng.minibatch_gradient(*Y, b_div=B)
    scale = np.abs(gxy).max()
    np.testing.assert_allclose(gxy, gx + gy, rtol=1e-4, atol=1e-5 * scale)


def test_ppo_update_config3_vs_oracle(wk, orc):
    """BASELINE config 3 shape: 4,096 walkers, rollout T = 8 (pool 32,768), M = 4,096,
    one epoch = 8 minibatches of 4,096 samples, each gradient -> ordered reduction -> Adam;
    the oracle replays the same Feistel minibatch sequence with its sequential Train(Batch).

    Adam normalises each step (at t = 1, dw = -alpha sign(g)), so a parameter whose
    gradient is within fp32 re-association noise of zero may legitimately step the other
    way: the bar is <= 5e-6 on all but a handful of such parameters, each of which must
    have a near-zero oracle gradient, and the last minibatch's gradient itself within the
    gradient tolerance above."""
    n, T, M, E, upd = 4096, 8, 4096, 1, 7
    eng = wk.Engine(n, seed=SEED, Horizon=T, Minibatch=M, Epochs=E, RandomizeStart=1)
    ag = orc.Agent(seed=SEED)
    eng.set_weights(ag.params())
    eng.rollout(T)
    tr = eng.get_trajectory(T)
    cd, ad = eng.ppo_update(update_index=upd)
    pool = n * T
    S = tr["states"].reshape(pool, 12)
    A = tr["actions"].reshape(pool, 4)
    L = tr["logp"].reshape(pool, 4)
    G = tr["returns"].reshape(pool)
    Ad = tr["advantages"].reshape(pool)
    grads = []
    for e in range(E):
        key = orc.perm_key(SEED, upd, e)
        idx_all = np.array([orc.perm(i, pool, key) for i in range((pool // M) * M)])
        assert len(np.unique(idx_all)) == len(idx_all)  # without replacement
        for j in range(pool // M):
            idx = idx_all[j * M:(j + 1) * M]
            w_before = ag.params()
            og, ocd, oad, _ = ag.train_batch(S[idx], A[idx], L[idx], G[idx], Ad[idx], b_div=M)
            grads.append((og, w_before, idx))
    w_gpu, w_orc = eng.get_weights(), ag.params()
    diff = np.abs(w_gpu - w_orc)
    bad = np.nonzero(diff > 5e-6)[0]
    # every outlier is a sign flip of a near-zero gradient somewhere in the sequence
    small = np.zeros(wk.NPARAM, bool)
    for og, _, _ in grads:
        small |= np.abs(og) < 1e-4 * np.abs(og).max()
    assert len(bad) <= 16 and small[bad].all(), (len(bad), diff.max(), bad[:16])
    assert diff.max() <= 2 * 1e-3 * E * (pool // M)  # at most 2 alpha per Adam step
    m, v, t = eng.get_adam()
    assert t == E * (pool // M)
    # the last minibatch's gradient and diagnostics, recomputed by the GPU kernel from the
    # oracle's pre-step weights: the gradient tolerance of the test above
    og, w_before, idx = grads[-1]
    chk = wk.Engine(4, seed=SEED)
    chk.set_weights(w_before)
    g, gcd, gad, _ = chk.minibatch_gradient(S[idx], A[idx], L[idx], G[idx], Ad[idx], b_div=M)
    g64, asum, _, _, _ = ref64.train_batch_grad64(w_before, S[idx], A[idx], L[idx], G[idx],
                                                  Ad[idx], M)
    _check_against_f64(g, og, g64, asum)
    assert cd == pytest.approx(ocd, rel=1e-3, abs=1e-6)
    assert ad == pytest.approx(oad, rel=1e-3, abs=1e-6)


def test_grad_kernel_selection(wk, monkeypatch):
    """wk_grad_kernel: the tile-parallel kernel below 32,768 samples per launch (one team per
    block up to 4,096), the producer / consumer kernel from there; WK_GRAD_IMPL (read at
    wk_create) overrides"""
    eng = wk.Engine(256, seed=SEED, Horizon=64, Minibatch=8192)
    assert eng.grad_kernel() == "k_ppo_grad_tp"
    assert eng.grad_kernel(4096) == "k_ppo_grad_tp1"
    assert eng.grad_kernel(4097) == "k_ppo_grad_tp"
    assert eng.grad_kernel(32767) == "k_ppo_grad_tp"
    assert eng.grad_kernel(32768) == "k_ppo_grad_ws"
    assert eng.grad_kernel(65536) == "k_ppo_grad_ws"
    monkeypatch.setenv("WK_GRAD_IMPL", "mf")
    assert wk.Engine(4, seed=SEED).grad_kernel(8192) == "k_ppo_grad_mfma"
    assert eng.grad_kernel(8192) == "k_ppo_grad_tp"  # per context
