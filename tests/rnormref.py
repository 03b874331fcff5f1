"""numpy restatement of the reward normalisation (include/wk_api.h, wk_reward_norm_*;
csrc/wk_rnorm.hip): the fp32 recurrence op for op, the batch's sums exactly (math.fsum), Chan's
merge in double, the scale formula and the apply rule.  The engine's sums have another (fixed)
association than fsum; `bounds` gives the standard bound for a sum in any order."""
import math

import numpy as np

F = np.float32


def scan(rewards, dones, gamma, acc0=None):
    """The scan over a [T][n] trajectory: per walker, forward over t, x = r + (a * gamma) in fp32
    (two roundings, no fused multiply-add); a finite x is a sample and the new carry, any other x
    is counted and zeroes the carry; a terminal row zeroes the carry.  Returns (acc [n] fp32, the
    samples as a list of Python floats in (walker, t) order, the non-finite count)."""
    r = np.asarray(rewards, F)
    d = np.asarray(dones)
    T, n = r.shape
    g = F(gamma)
    a = np.zeros(n, F) if acc0 is None else np.array(acc0, F).reshape(n).copy()
    per = [[] for _ in range(n)]
    bad = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            x = (r[t] + (a * g).astype(F)).astype(F)
            fin = np.isfinite(x)
            bad += int((~fin).sum())
            for e in np.nonzero(fin)[0]:
                per[e].append(float(x[e]))
            a = np.where(fin, x, F(0)).astype(F)
            a = np.where(d[t] != 0, F(0), a).astype(F)
    return a, [x for lst in per for x in lst], bad


def batch_moments(samples):
    """(cnt_b, s1, s2): the count and the exact sums of x and x^2, rounded once (fsum; the double
    square of a float is exact)"""
    return len(samples), math.fsum(samples), math.fsum(x * x for x in samples)


def merge(count, mean, m2, cnt_b, s1, s2):
    """Chan's merge of a batch's (cnt_b, s1, s2) into the running (count, mean, m2), in double"""
    if cnt_b == 0:
        return count, mean, m2
    mean_b = s1 / cnt_b
    m2_b = max(0.0, s2 - s1 * mean_b)
    delta = mean_b - mean
    tot = float(count) + float(cnt_b)
    mean = mean + delta * float(cnt_b) / tot
    m2 = m2 + (m2_b + delta * delta * float(count) * float(cnt_b) / tot)
    return count + cnt_b, mean, m2


def scale_of(count, m2, epsilon):
    """(var, scale): var = m2 / count (0 without samples); scale = (float)(1 / sqrt(var +
    (double)epsilon)), 1 without samples or when that is not finite and positive"""
    if count <= 0:
        return 0.0, F(1)
    var = m2 / float(count)
    with np.errstate(all="ignore"):
        s = F(np.float64(1.0) / np.sqrt(np.float64(var) + np.float64(F(epsilon))))
    return var, (s if np.isfinite(s) and s > 0 else F(1))


def apply(rewards, scale, clip):
    """(scaled rewards, rows the clamp changed): y = r * scale, one fp32 product; |y| > clip gives
    copysign(clip, y); a NaN stays"""
    r = np.asarray(rewards, F)
    with np.errstate(all="ignore"):
        y = (r * F(scale)).astype(F)
        hit = np.abs(y) > F(clip)
    return np.where(hit, np.copysign(F(clip), y), y).astype(F), int(hit.sum())


class Running:
    """The state an enabled context holds: acc [n], (count, mean, m2), scale -- and the sums of
    |x| and x^2 over every sample so far, for `bounds`."""

    def __init__(self, n, gamma, clip=10.0, epsilon=1e-8):
        self.n, self.gamma, self.clip, self.epsilon = n, gamma, clip, epsilon
        self.acc = np.zeros(n, F)
        self.count, self.mean, self.m2 = 0, 0.0, 0.0
        self.var, self.scale = 0.0, F(1)
        self.nonfinite = 0
        self.sum_abs, self.sum_sq = 0.0, 0.0

    def update(self, rewards, dones):
        """the full pass; returns (scaled rewards, clipped)"""
        self.acc, xs, self.nonfinite = scan(rewards, dones, self.gamma, self.acc)
        self.count, self.mean, self.m2 = merge(self.count, self.mean, self.m2, *batch_moments(xs))
        self.var, self.scale = scale_of(self.count, self.m2, self.epsilon)
        self.sum_abs += math.fsum(abs(x) for x in xs)
        self.sum_sq += math.fsum(x * x for x in xs)
        return apply(rewards, self.scale, self.clip)

    def bounds(self):
        """(mean, m2): 2 N 2^-53 sum|x| / N and 2 N 2^-53 sum x^2, N the samples so far -- the
        bound of a sum in any order, the factor 2 for the merge's few extra roundings"""
        u = 2.0 ** -53
        return 2.0 * u * self.sum_abs, 2.0 * self.count * u * self.sum_sq
