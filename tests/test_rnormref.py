"""CPU: tests/rnormref.py, the numpy restatement of the reward normalisation that
tests/test_gpu_rnorm.py holds the kernels to -- its own invariants, with no library."""
import math

import numpy as np

import rnormref

F = np.float32
GAMMA = 0.9


def _traj(seed, T, n, p_done=0.1):
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((T, n)) * 20.0 + 3.0).astype(F)
    d = (rng.random((T, n)) < p_done).astype(np.uint8)
    return r, d


def test_merging_two_batches_equals_one_batch_of_both():
    rng = np.random.default_rng(1)
    a = [float(F(x)) for x in rng.standard_normal(700) * 30.0 + 50.0]
    b = [float(F(x)) for x in rng.standard_normal(45) * 5.0 - 200.0]
    one = rnormref.merge(0, 0.0, 0.0, *rnormref.batch_moments(a + b))
    two = rnormref.merge(*rnormref.merge(0, 0.0, 0.0, *rnormref.batch_moments(a)), *rnormref.batch_moments(b))
    xs = a + b
    N, sum_abs, sum_sq = len(xs), math.fsum(abs(x) for x in xs), math.fsum(x * x for x in xs)
    assert one[0] == two[0] == N
    # double rounding: a few roundings of the mean, and of sums as large as sum x^2 for m2
    assert abs(one[1] - two[1]) <= 8 * 2.0 ** -53 * sum_abs / N
    assert abs(one[2] - two[2]) <= 8 * 2.0 ** -53 * sum_sq
    # and both are the moments: against the two-pass formula on the exact mean
    mu = math.fsum(xs) / N
    m2 = math.fsum((x - mu) ** 2 for x in xs)
    assert abs(one[1] - mu) <= 4 * 2.0 ** -53 * sum_abs / N
    assert abs(one[2] - m2) <= 8 * 2.0 ** -53 * sum_sq


def test_carry_across_a_split_equals_the_unsplit_trajectory():
    r, d = _traj(2, 24, 37)
    whole, xs, bad = rnormref.scan(r, d, GAMMA)
    for cut in (1, 7, 23):
        a1, x1, b1 = rnormref.scan(r[:cut], d[:cut], GAMMA)
        a2, x2, b2 = rnormref.scan(r[cut:], d[cut:], GAMMA, a1)
        assert a2.tobytes() == whole.tobytes()
        assert sorted(x1 + x2) == sorted(xs) and b1 + b2 == bad == 0
    assert whole.dtype == F and len(xs) == r.size


def test_a_done_row_zeroes_the_carry():
    r = np.array([[1.0, 1.0], [2.0, 2.0], [4.0, 4.0]], F)
    d = np.array([[0, 0], [1, 0], [0, 0]], np.uint8)
    acc, xs, _ = rnormref.scan(r, d, 0.5)
    # walker 0: 1, 2 + 0.5, done, 4; walker 1: 1, 2.5, 4 + 1.25
    assert acc.tolist() == [4.0, 5.25]
    assert xs == [1.0, 2.5, 4.0, 1.0, 2.5, 5.25]
    acc, _, _ = rnormref.scan(r, np.array([[0, 0], [0, 0], [1, 0]], np.uint8), 0.5)
    assert acc.tolist() == [0.0, 5.25]  # a done on the last row
    acc, xs, _ = rnormref.scan(r, np.ones((3, 2), np.uint8), 0.5, acc0=[100.0, 0.0])
    assert acc.tolist() == [0.0, 0.0] and xs[:3] == [51.0, 2.0, 4.0]  # the start value counts once


def test_nonfinite_samples_are_left_out_and_counted():
    r = np.array([[1.0], [np.nan], [2.0], [np.inf], [-np.inf], [3.0]], F)
    acc, xs, bad = rnormref.scan(r, np.zeros((6, 1), np.uint8), 0.5)
    assert bad == 3 and xs == [1.0, 2.0, 3.0] and acc.tolist() == [3.0]  # each one zeroes the carry
    # an overflow of the recurrence itself is non-finite too
    big = np.full((2, 1), np.finfo(F).max, F)
    acc, xs, bad = rnormref.scan(big, np.zeros((2, 1), np.uint8), 1.0)
    assert bad == 1 and len(xs) == 1 and acc.tolist() == [0.0]
    st = rnormref.Running(1, 0.5)
    y, clipped = st.update(r, np.zeros((6, 1), np.uint8))
    assert st.count == 3 and st.nonfinite == 3 and st.mean == 2.0 and st.m2 == 2.0
    # NaN stays, the infinities clamp
    assert np.isnan(y[1, 0]) and y[3, 0] == 10.0 and y[4, 0] == -10.0 and clipped == 2


def test_scale_is_one_with_no_samples():
    assert rnormref.scale_of(0, 0.0, 1e-8) == (0.0, F(1))
    st = rnormref.Running(3, GAMMA)
    y, clipped = st.update(np.full((2, 3), np.nan, F), np.zeros((2, 3), np.uint8))
    assert st.count == 0 and st.nonfinite == 6 and st.scale == F(1) and st.var == 0.0 and clipped == 0
    # a zero variance with epsilon 0 divides by zero: not finite, so 1
    assert rnormref.scale_of(5, 0.0, 0.0) == (0.0, F(1))
    var, s = rnormref.scale_of(4, 16.0, 0.0)
    assert (var, s) == (4.0, F(0.5)) and s.dtype == F


def test_apply_rule():
    r = np.array([3.0, -3.0, 0.5, np.nan, np.inf, -np.inf, 0.0], F)
    y, clipped = rnormref.apply(r, F(2.0), 5.0)
    assert y[:3].tolist() == [5.0, -5.0, 1.0] and np.isnan(y[3]) and y[4:].tolist() == [5.0, -5.0, 0.0]
    assert clipped == 4 and y.dtype == F
    y, clipped = rnormref.apply(r, F(2.0), np.inf)
    assert clipped == 0 and y[4:6].tolist() == [np.inf, -np.inf]
