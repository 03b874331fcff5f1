"""Restatement of the returns / advantages scans -- test infrastructure only (numpy).

  * returns32(mode, ...): float32, operation for operation as the kernels' one scan
    (returns_scan<STD>, csrc/wk_returns.hip): mode 0 restates k_returns (the reference's
    PPOAgent.cs:414-498, whose GAE chain is never carried and whose scans start from 0), mode 1
    restates k_returns_std (chained GAE(lambda), the scan started from vlast).  The library is built
    without contraction, so every product and sum below rounds once, as on the GPU.
  * returns64(mode, ...): the same scans in float64.
  * normalize32: k_normalize (PPOAgent.cs:461-472; mean and variance accumulate in double).
  * normalize_case: the advantages the k_normalize tests share between the GPU comparison and the
    CPU proof that the offset kind tells a float32 accumulation from the double one.

Arrays are [T][n] (rows = env-steps), vlast is [n]; every walker's scan is independent, so the
scans are vectorised over the walkers and sequential over the rows.
"""
import numpy as np

F = np.float32


def _scan(mode, use_gae, gamma, lam, r, v, d, vlast, ft):
    r = np.asarray(r, ft)
    v = np.asarray(v, ft)
    d = np.asarray(d).astype(bool)
    T, n = r.shape
    gamma, lam = ft(gamma), ft(lam)
    zero = np.zeros(n, ft)
    start = zero.copy() if mode == 0 else np.asarray(vlast, ft).reshape(n).copy()
    ret = np.empty((T, n), ft)
    adv = np.empty((T, n), ft)
    with np.errstate(all="ignore"):
        if not use_gae:
            disc = start
            for t in range(T - 1, -1, -1):
                disc = np.where(d[t], zero, disc)  # assignment, not a multiply
                disc = r[t] + (disc * gamma)
                ret[t] = disc
                adv[t] = disc - v[t]
        else:
            next_value, next_gae = start, zero.copy()
            gl = gamma * lam  # gamma * lambda * nextGae parses as (gamma * lambda) * nextGae
            for t in range(T - 1, -1, -1):
                next_value = np.where(d[t], zero, next_value)
                if mode == 1:
                    next_gae = np.where(d[t], zero, next_gae)
                cur = v[t]
                delta = r[t] + (gamma * next_value) - cur
                gae = delta + (gl * next_gae)
                adv[t] = gae
                ret[t] = gae + cur
                next_value = cur
                if mode == 1:  # mode 0: the reference never assigns nextGae
                    next_gae = gae
    assert ret.dtype == ft and adv.dtype == ft
    return ret, adv


def returns32(mode, use_gae, gamma, lam, r, v, d, vlast=None):
    """(ret, adv) in float32, bit for bit what the kernels compute"""
    return _scan(mode, use_gae, gamma, lam, r, v, d, vlast, np.float32)


def returns64(mode, use_gae, gamma, lam, r, v, d, vlast=None):
    return _scan(mode, use_gae, gamma, lam, r, v, d, vlast, np.float64)


def normalize32(x, eps_clip):
    """k_normalize on the flattened advantages: (x - mean) / (std + Epsilon)"""
    x = np.asarray(x, F)
    flat = x.reshape(-1)
    mean = F(flat.astype(np.float64).sum() / flat.size)
    dv = (flat - mean).astype(np.float64)
    sd = F(np.sqrt((dv * dv).sum() / flat.size))
    return ((flat - mean) / (sd + F(eps_clip))).astype(F).reshape(x.shape)


NORMALIZE_SIZES = [(1, 1), (2, 1), (1023, 1), (1024, 1), (1025, 1), (33, 31), (65, 64)]  # (n, T)
NORMALIZE_KINDS = ["standard", "offset", "constant"]


def normalize_case(kind, n, T):
    """[T][n] float32 advantages: standard normal; mean about 3e4 with spread 1 (the mean dwarfs the
    spread: what the reference's double Average / Sum exists for); constant (sd = 0)"""
    g = np.random.default_rng(100 * n + T)
    z = g.standard_normal((T, n))
    if kind == "standard":
        return z.astype(F)
    if kind == "offset":
        return (3.0e4 + z).astype(F)
    assert kind == "constant"
    return np.full((T, n), 30000.37, F)
