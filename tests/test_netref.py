"""CPU: the general numpy restatement used by the general networks' GPU tests (tests/netref.py)
agrees, for the default strings, with the float64 restatement of the built-in network
(tests/ref64.py) and with the oracle's fp32 forward pass."""
import numpy as np
import pytest

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
