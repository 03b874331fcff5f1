"""GPU: the four built-in matrix-core gradient kernels of csrc/wk_ppo_mfma.hip -- k_ppo_grad_ws,
k_ppo_grad_tp<2>, k_ppo_grad_tp<1> and k_ppo_grad_mfma, each forced with WK_GRAD_IMPL (read at
wk_create) -- where tests/test_gpu_grad_scale.py and tests/test_gpu_parity.py do not reach:

  A. training-like inputs (net_cases.surrogate_draw: actions within 1.5 std of the mean, ratios
     cycling through all six cells of the clipped surrogate, |Adv| >= 0.1, so every sample carries
     its share of the actor gradient) at the occupancy edges of every kernel (net_cases.GRAD_EDGE_BS)
     against float64, and a non-default Epsilon and log-std, set in the configuration and at run
     time;
  B. one live sample in every kind of slot of a 16,391-sample launch (every lane of a chunk, the
     units of a block, the last unit of a pass and the first of the next, the ragged last chunk):
     the same values at every position, and those of the sample alone;
  C. the skip rule (exp(logp_old) == 0) on the first row, a whole chunk, the first row of a unit's
     second chunk and every row, and with non-finite values in the skipped rows: no bit changes;
  D. a slab buffer that a larger launch has filled, and every call of A repeated;
  E. the permuted gather of wk_ppo_update (use_perm = 1, base > 0): Adam's moments after a whole
     update at a learning rate of 0 are, bit for bit, those of the same kernel's gradients of the
     same rows, gathered on the host and folded through clipref.

Inputs: tests/net_cases.py; tests/test_netref.py re-checks every condition on them without a GPU.
Bars: the gradient bar |g - g64| <= 1e-5 * sum|t| + 1e-7 * max|g64| and the diagnostics' 1e-5 *
(|x| + 1) of tests/test_gpu_net_edges.py (`_check`), or equality.  Each case prints its worst
ratio (pytest -s; measured values: DESIGN.md "Built-in gradient kernels at their edges").
"""
import functools

import numpy as np
import pytest

import clipref
import net_cases
import netref
from test_gpu_net_edges import _bits, _check, _same_bits

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 20250905
IMPLS = ["ws", "tp", "tp1", "mf"]
CD, AD = netref.NETS["default"]
NC = netref.n_params(CD)
# chunks that one pass of every unit takes: the row 16 * UNITS[impl] is the first of unit 0's
# second chunk (256 blocks of 4 pairs / waves, of 2 teams, of 1 team)
UNITS = {"ws": 1024, "mf": 1024, "tp": 512, "tp1": 256}


def _eng(wk, monkeypatch, impl, n=4, **cfg):
    monkeypatch.setenv("WK_GRAD_IMPL", impl)
    eng = wk.Engine(n, seed=SEED, **cfg)
    want = {"ws": "k_ppo_grad_ws", "tp": "k_ppo_grad_tp", "tp1": "k_ppo_grad_tp1", "mf": "k_ppo_grad_mfma"}
    assert eng.grad_kernel(8192) == want[impl]
    return eng


def _f64(w, batch, b_div, **kw):
    return netref.train_batch_grad64(CD, AD, w, *batch, b_div, **kw)


@functools.lru_cache(maxsize=None)
def _ref(B, variant="default"):
    """(weights, batch, float64 reference) of a GRAD_EDGE_CASES entry, computed once; read-only"""
    w, batch = net_cases.grad_edge_case(B, variant)
    ref = _f64(w, batch, B, **net_cases.grad_edge_params(variant)[1])
    for x in (w, *batch, ref[0], ref[1]):
        x.setflags(write=False)
    return w, batch, ref


# ---- A. training-like inputs at the occupancy edges ----
@pytest.mark.parametrize("B", net_cases.GRAD_EDGE_BS)
@pytest.mark.parametrize("impl", IMPLS)
def test_training_like_edge_case_vs_f64(wk, monkeypatch, impl, B):
    w, batch, ref = _ref(B)
    eng = _eng(wk, monkeypatch, impl)
    eng.set_weights(w)
    got = eng.minibatch_gradient(*batch)
    assert got[3] == 0
    _check(f"grad {impl:3s} B {B:6d}", got, ref)
    _same_bits(got, eng.minibatch_gradient(*batch))  # D: the repeat on one context


@pytest.mark.parametrize("B", net_cases.TIGHT_BS)
@pytest.mark.parametrize("impl", IMPLS)
def test_non_default_epsilon_and_log_std(wk, monkeypatch, impl, B):
    """Epsilon = 0.1 at a log-std of -0.5, ratios 0.85 / 0.95 / 1.05 / 1.15: from the configuration
    and through set_log_std on a context created at the default -1.0; the two bit for bit"""
    w, batch, ref = _ref(B, "tight")
    t = net_cases.TIGHT
    cfg = _eng(wk, monkeypatch, impl, Epsilon=t["eps_clip"], LogStandardDeviation=t["log_std"])
    cfg.set_weights(w)
    a = cfg.minibatch_gradient(*batch)
    _check(f"grad {impl:3s} B {B:6d} eps 0.1 log-std -0.5 (config)", a, ref)
    run = _eng(wk, monkeypatch, impl, Epsilon=t["eps_clip"])
    run.set_weights(w)
    at_default = run.minibatch_gradient(*batch)
    run.set_log_std(t["log_std"])
    b = run.minibatch_gradient(*batch)
    _check(f"grad {impl:3s} B {B:6d} eps 0.1 log-std -0.5 (set_log_std)", b, ref)
    _same_bits(a, b)
    assert (_bits(at_default[0]) != _bits(b[0])).any()
    _same_bits(a, cfg.minibatch_gradient(*batch))


# ---- B. one live sample at every kind of position ----
@functools.lru_cache(maxsize=None)
def _sweep_base():
    w, batch = net_cases.surrogate_draw("default", net_cases.SWEEP_SEED, B=net_cases.SWEEP_B)
    S, A, L, G, Ad = (x.copy() for x in batch)
    live = tuple(x[:1].copy() for x in (S, A, L, G, Ad))
    L[:, 2] = -200.0
    for x in (w, S, A, L, G, Ad, *live):
        x.setflags(write=False)
    return w, (S, A, L, G, Ad), live


def _sweep_batch(p):
    _, dead, live = _sweep_base()
    out = tuple(x.copy() for x in dead)
    for x, row in zip(out, live):
        x[p] = row[0]
    return out


@pytest.mark.parametrize("impl", IMPLS)
def test_one_live_sample_at_every_position(wk, monkeypatch, impl):
    """Every row of a 16,391-sample launch is skipped (logp_old[i, 2] = -200) but one, which holds
    the same five fields wherever it stands.  A skipped row contributes selected zeros, sums with
    zeros are exact in any association, and a sample's forward pass touches only its own column of
    the matrix products: so the gradient, both diagnostics and the skip count are the same values
    (np.array_equal: +0 and -0 alike) at every position, and equal the launch of the live row
    alone at the same divisor."""
    B = net_cases.SWEEP_B
    w, _, live = _sweep_base()
    eng = _eng(wk, monkeypatch, impl)
    eng.set_weights(w)
    alone = eng.minibatch_gradient(*live, b_div=B)
    assert alone[3] == 0 and alone[0][:NC].any() and alone[0][NC:].any() and alone[1] != 0 and alone[2] != 0
    _check(f"grad {impl:3s} the live row alone", alone, _f64(w, live, B))
    wrong = []
    for p in net_cases.SWEEP_POSITIONS:
        g, cd, ad, sk = eng.minibatch_gradient(*_sweep_batch(p))
        same = np.array_equal(g, alone[0]) and cd == alone[1] and ad == alone[2] and sk == B - 1
        if not same:
            wrong.append((p, int((g != alone[0]).sum()), cd, ad, sk))
    print(f"grad {impl:3s} live row at {len(net_cases.SWEEP_POSITIONS)} positions of B {B}: {len(wrong)} differ")
    assert not wrong, (impl, alone[1:], wrong)


# ---- C. the skip rule, with poison ----
def _skip_rows(impl, pattern, B):
    """None where the pattern does not exist at B"""
    if pattern == "unit2":
        return np.array([16 * UNITS[impl]]) if B > 16 * UNITS[impl] else None
    return net_cases.skip_rows(pattern, B)


SKIPS = [(impl, B, p) for impl in IMPLS for B in (33, 16385) for p in ("first", "tile", "unit2", "all")
         if _skip_rows(impl, p, B) is not None]
assert len(SKIPS) == 4 * 7


@pytest.mark.parametrize("impl,B,pattern", SKIPS)
def test_skipped_rows_are_inert(wk, monkeypatch, impl, B, pattern):
    """rows with logp_old[i, 2] = -200 (exp == 0 in fp32): the reference `continue`s before it
    touches such a sample, so what the row holds otherwise -- here NaN states and returns, +inf
    actions, -inf advantages -- must change no bit of any output.  `unit2`: the first row of the
    second chunk of unit 0 (B = 16,385, where every kernel has one).  On B = 33 the sequential
    kernel (train_batch) takes the poisoned bytes as well.  (Before the kernels evaluated the rule
    at the top of the chunk and zeroed such a row's states, all 28 poisoned launches returned NaN
    in 6,084 of the 6,149 gradient entries: the selected zero losses met the row's activations.)"""
    rows = _skip_rows(impl, pattern, B)
    w, base, _ = _ref(B)
    batch = net_cases.with_skips(base, rows)
    ref = _f64(w, batch, B)
    assert ref[4] == len(rows)
    eng = _eng(wk, monkeypatch, impl)
    eng.set_weights(w)
    got = eng.minibatch_gradient(*batch)
    assert got[3] == len(rows)
    _check(f"grad {impl:3s} B {B:6d} skip {pattern:6s}", got, ref)
    if pattern == "all":
        assert not got[0].any() and got[1] == 0.0 and got[2] == 0.0
    poisoned = net_cases.with_skips(base, rows, poison=True)
    _same_bits(got, eng.minibatch_gradient(*poisoned))
    if B == 33:
        seq = eng.train_batch(*poisoned, apply_adam=False)
        _check(f"grad seq B {B:6d} skip {pattern:6s} poisoned", seq, ref)


# ---- D. the slab buffer after a larger launch ----
@pytest.mark.parametrize("impl", IMPLS)
def test_stale_slabs_change_nothing(wk, monkeypatch, impl):
    """B = 16,385 fills every slab the kernel can write (256); B = 17 at other weights then writes
    one or two of them, and the reduction must not see what the others hold"""
    w, big, _ = _ref(16385)
    w17, small, ref17 = _ref(17)
    assert (_bits(w) != _bits(w17)).any()
    eng = _eng(wk, monkeypatch, impl)
    eng.set_weights(w)
    first = eng.minibatch_gradient(*big)
    eng.set_weights(w17)
    mid = eng.minibatch_gradient(*small)
    eng.set_weights(w)
    third = eng.minibatch_gradient(*big)
    _same_bits(first, third)
    fresh = _eng(wk, monkeypatch, impl)
    fresh.set_weights(w17)
    _same_bits(mid, fresh.minibatch_gradient(*small))
    _check(f"grad {impl:3s} after B 16385: B 17", mid, ref17)


# ---- E. the permuted gather ----
@pytest.mark.parametrize("shape", sorted(net_cases.PERM_CASES))
@pytest.mark.parametrize("impl", IMPLS)
def test_permuted_gather_bit_for_bit(wk, orc, monkeypatch, impl, shape):
    """wk_ppo_update at a learning rate of 0 (the weights and their operand image never move):
    every minibatch is the keyed permutation's rows base .. base + M - 1, gathered by the kernel.
    A second context of the same kernel, given the same rows gathered on the host, runs the same
    kernel on the same samples in the same slots: its gradients, folded through the Adam moments
    (clipref, held to the fused Adam bit for bit by tests/test_gpu_clip.py), are the update's m and
    v bit for bit, and the update's diagnostics are the last minibatch's."""
    n, T, M, E = shape
    pool, nmb = n * T, (n * T) // M
    w, traj = net_cases.perm_trajectory(shape)
    eng = _eng(wk, monkeypatch, impl, n=n, Horizon=T, Minibatch=M, Epochs=E)
    eng.set_weights(w)
    eng.set_trajectory(**traj)
    eng.compute_returns()
    tr = eng.get_trajectory(T)
    rows = (tr["states"].reshape(pool, 12), tr["actions"].reshape(pool, 4), tr["logp"].reshape(pool, 4),
            tr["returns"].reshape(pool), tr["advantages"].reshape(pool))
    np.testing.assert_array_equal(_bits(rows[0]), _bits(traj["states"].reshape(pool, 12)))
    m, v, t = eng.get_adam()
    assert t == 0 and not m.any() and not v.any()
    eng.set_learning_rate(0.0)
    cd, ad = eng.ppo_update(update_index=net_cases.PERM_UPDATE)
    np.testing.assert_array_equal(_bits(eng.get_weights()), _bits(w))

    chk = _eng(wk, monkeypatch, impl)
    chk.set_weights(w)
    rm, rv, steps, last = np.zeros(w.size, F), np.zeros(w.size, F), 0, None
    for e in range(E):
        idx_all = orc.perm_batch(nmb * M, pool, orc.perm_key(SEED, net_cases.PERM_UPDATE, e))
        for j in range(nmb):
            idx = idx_all[j * M:(j + 1) * M]
            last = chk.minibatch_gradient(*(x[idx] for x in rows), b_div=M)
            assert last[3] == 0
            steps += 1
            _, rm, rv, _, _ = clipref.clip_adam32(w, rm, rv, last[0], steps, NC, 0.0, alpha=0.0, scales=(1.0, 1.0))
    m, v, t = eng.get_adam()
    assert t == steps == E * nmb
    print(f"grad {impl:3s} pool {pool} M {M} E {E}: {steps} Adam steps, "
          f"{int((_bits(m) != _bits(rm)).sum())} m and {int((_bits(v) != _bits(rv)).sum())} v entries differ")
    np.testing.assert_array_equal(_bits(m), _bits(rm))
    np.testing.assert_array_equal(_bits(v), _bits(rv))
    assert rm.any() and rv.any()
    assert _bits([cd, ad]).tolist() == _bits([last[1], last[2]]).tolist()
