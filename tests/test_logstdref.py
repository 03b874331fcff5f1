"""CPU: tests/logstdref.py, the float64 restatement the GPU tests of the log-std pass rest on.

  * grad64 against the central finite difference of the float64 mean surrogate in s (h = 1e-5),
    bounded against mean|term| and never against the gradient: on these cases |sum term| /
    sum|term| goes as low as 0.009 (default, P = 15).  Tolerance 1e-8 mean|term|; the truncation
    error of the central difference is h^2 / 6 times the third derivative, and every ratio is
    0.2 from a clip bound, so no selection flips within h.
  * adam_scalar: the first step from zero moments, the clamp, the no-step rule.
  * the tight case: grad64 > 0, the loss falls as s falls.
"""
import math

import numpy as np
import pytest

import logstdref
import statsref

F = np.float32
NAMES = ("default", "odd", "edge16")
PS = (1, 15, 16, 17, 33, 16385)


def _inputs(name, P, traj=None):
    """the case's float64 mean and fp32 actions, logp_old and advantages (reward - old value, as
    the engine forms them for all-terminal rows)"""
    _, base = statsref.case(name, P)
    traj = base if traj is None else traj
    adv = (traj["rewards"].reshape(P) - traj["values"].reshape(P)).astype(F)
    return logstdref.mean64(name, P), traj["actions"].reshape(P, 4), traj["logp"].reshape(P, 4), adv


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("P", PS)
def test_grad64_is_the_derivative(name, P):
    m, A, L, adv = _inputs(name, P)
    s, h = -1.0, 1e-5
    g, abs_sum, term = logstdref.grad64(m, A, L, adv, s)
    fd = -(logstdref.surrogate64(m, A, L, adv, s + h) - logstdref.surrogate64(m, A, L, adv, s - h)) / (2 * h)
    scale = abs_sum / term.size
    print(f"{name}/P={P}: grad {g:.6g}, |grad - fd| / mean|term| = {abs(g - fd) / scale:.3g}, "
          f"|sum term| / sum|term| = {abs(term.sum()) / abs_sum:.3g}")
    assert term.shape == (P, 4) and abs(g - fd) <= 1e-8 * scale


def test_grad64_skips_and_empty():
    """skipped rows leave the gradient of the others; no counted row gives NaN"""
    name, P = "default", 33
    _, base = statsref.case(name, P)
    rows = np.arange(16, 32)
    m, A, L, adv = _inputs(name, P, statsref.with_skips(base, rows))
    keep = np.setdiff1d(np.arange(P), rows)
    g, a, term = logstdref.grad64(m, A, L, adv, -1.0)
    g2, a2, _ = logstdref.grad64(m[keep], A[keep], L[keep], adv[keep], -1.0)
    assert (g, a) == (g2, a2) and term.shape == (P - 16, 4)
    m, A, L, adv = _inputs(name, P, statsref.with_skips(base, np.arange(P)))
    assert math.isnan(logstdref.grad64(m, A, L, adv, -1.0)[0])


def test_terms32_recovers_zz():
    """terms32's zz = 2 (lp_const - lp) lies in zz_bracket of the same lp, and the bracket holds
    the zz the lp was formed from"""
    name, P = "odd", 33
    m, A, L, adv = _inputs(name, P)
    std, c = logstdref.consts32(-1.0)
    assert abs(float(std) - math.exp(-1.0)) < 1e-7 and abs(float(c) - (1.0 - logstdref.LOG_SQRT_2PI)) < 1e-7
    fr = ((A - m.astype(F)) / std).astype(F)
    zz = (fr * fr).astype(F)
    lp = (c - (zz / F(2)).astype(F)).astype(F)
    w, z2 = logstdref.terms32(lp, L, adv, c)
    lo, hi = logstdref.zz_bracket(lp, c)
    assert (lo <= zz).all() and (zz <= hi).all() and (lo <= z2).all() and (z2 <= hi).all()
    assert w.dtype == F and z2.dtype == F
    # against float64 at fp32's precision
    term64 = logstdref.grad64(m, A, L, adv, -1.0)[2]
    np.testing.assert_allclose(w.astype(np.float64) * (z2.astype(np.float64) - 1), term64, rtol=0,
                               atol=2e-5 * np.abs(term64).max() + 1e-5)


def test_adam_scalar():
    b1, b2, eps = float(F(0.9)), float(F(0.999)), float(F(1e-8))
    for g in (3.0, -0.02):
        s, m, v, t, clamped, stepped = logstdref.adam_scalar(-1.0, 0.0, 0.0, 0, g, 1e-2, b1, b2, eps, -4.0, 1.0)
        # m / (1 - b1) = g and sqrt(v / (1 - b2)) = |g|: the first step is lr sign(g)
        assert stepped and not clamped and t == 1
        assert abs(s - (-1.0 - 1e-2 * math.copysign(1.0, g))) <= 2.0 ** -23
        assert m == (1.0 - b1) * g and v == (1.0 - b2) * g * g
        assert s == float(F(s))  # an fp32 value
    # the clamp: a step past the bound lands on it and is counted
    hi = float(np.nextafter(F(-1.0), F(0)))
    s, m, v, t, clamped, stepped = logstdref.adam_scalar(-1.0, 0.0, 0.0, 0, -1.0, 1.0, b1, b2, eps, -4.0, hi)
    assert (s, t, clamped, stepped) == (hi, 1, True, True)
    s, *_, clamped, stepped = logstdref.adam_scalar(-1.0, 0.0, 0.0, 0, 1.0, 5.0, b1, b2, eps, -4.0, 1.0)
    assert (s, clamped, stepped) == (-4.0, True, True)
    # non-finite: nothing moves
    for g in (float("nan"), float("inf"), -float("inf")):
        assert logstdref.adam_scalar(-0.5, 0.1, 0.2, 7, g, 1e-2, b1, b2, eps, -4.0, 1.0) == \
            (-0.5, 0.1, 0.2, 7, False, False)


@pytest.mark.parametrize("name", NAMES)
def test_tight_case(name):
    """actions closer to the mean than std says, positive advantages: the gradient is positive
    and the loss falls as s falls; negated advantages turn both round"""
    P = 33
    for negated in (False, True):
        _, traj = logstdref.tight(name, P, negated=negated)
        m, A, L, adv = _inputs(name, P, traj)
        assert ((adv < 0) if negated else (adv > 0)).all()
        lp, _ = logstdref._lp64(m, A, -1.0)
        np.testing.assert_allclose(np.exp(lp - L), 1.0, rtol=0, atol=1e-6)  # every ratio 1
        g = logstdref.grad64(m, A, L, adv, -1.0)[0]
        loss = lambda s: -logstdref.surrogate64(m, A, L, adv, s)
        if negated:
            assert g < 0 and loss(-1.0 + 1e-3) < loss(-1.0)
        else:
            assert g > 0 and loss(-1.0 - 1e-3) < loss(-1.0)
