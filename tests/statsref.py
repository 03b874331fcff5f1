"""float64 restatement of wk_policy_stats' statistics on top of tests/netref.py, and the inputs of
tests/test_gpu_stats.py -- test infrastructure only (numpy).  tests/test_statsref.py checks the
restatement and the conditions the GPU tests' exact counts rest on without a GPU.

A case is a trajectory buffer of P = n * T rows, [t][e] order, for one of netref.NETS:
  * weights and states drawn as tests/net_cases.py draws them; actions near the float64 mean;
  * logp_old = lp64 - log(rho) per entry, rho cycling through net_cases.RHO = {0.5, 0.9, 1.1, 1.5},
    so the float64 ratio of an entry is rho up to the rounding of logp_old: two cells outside the
    clip bounds 1 +- 0.3, two inside, none within 1e-3 of a bound;
  * advantages of both signs, returns N(0, 5^2).
The engine computes returns and advantages itself (ReturnsMode 0, Monte Carlo), so the case
hands it every row as a terminal step (done = 1): ret = reward, adv = reward - value, and the
rewards / old values are chosen to give the drawn returns and advantages.  The tests read the
fp32 returns and advantages back from the buffer; those are the reference's inputs.
"""
import functools

import numpy as np

import net_cases
import netref

F = np.float32
EPS_CLIP = 0.3
STD = float(F(np.exp(F(-1.0))))
SMALL_P = (1, 15, 16, 17, 33)
# (n walkers, T rows per walker) of every P the tests use
SHAPES = {1: (1, 1), 15: (5, 3), 16: (4, 4), 17: (17, 1), 33: (11, 3), 16385: (145, 113),
          32769: (2979, 11)}
SKIP_PATTERNS = ("first", "tile", "block1", "all")


def large_p(family):
    """one row more than a whole number of grid passes (here: one pass).
    built-in (k_ppo_stats): the grid is capped at STATS_MAX_BLOCKS blocks of STATS_WAVES waves, one
    16-row chunk per wave and pass -- 512 * 4 * 16 = 32,768 rows; at 32,769 the first wave of the
    first block takes a second chunk, of one row.
    general (k_net_stats): at most NET_MAX_BLOCKS one-wave blocks of equally many consecutive
    16-row tiles -- 1,024 * 16 = 16,384 rows; at 16,385 block ownership goes from one tile to two."""
    import wk
    if family == "builtin":
        return wk.STATS_MAX_BLOCKS * wk.STATS_WAVES * wk.STATS_ROWS + 1
    return wk.NET_MAX_BLOCKS * wk.STATS_ROWS + 1


def second_block_row(family, P):
    """the first row the second block reads, or None when one block does everything"""
    import wk
    tiles = (P + 15) // 16
    if family == "builtin":  # block b, wave w starts at chunk 4 b + w
        return 16 * wk.STATS_WAVES if tiles > wk.STATS_WAVES else None
    tpb = (tiles + wk.NET_MAX_BLOCKS - 1) // wk.NET_MAX_BLOCKS
    return 16 * tpb if tiles > tpb else None


def skip_rows(pattern, family, P):
    """rows whose logp_old gets -200 in one dimension; None where the pattern does not exist"""
    if pattern == "first":
        return np.array([0])
    if pattern == "tile":
        return np.arange(16, 32) if P >= 32 else None
    if pattern == "block1":
        r = second_block_row(family, P)
        return None if r is None else np.array([r])
    return np.arange(P)


@functools.lru_cache(maxsize=None)
def case(name, P):
    """(weights, dict of the set_trajectory arrays [T, n, ...]), read-only and shared"""
    n, T = SHAPES[P]
    rng = np.random.default_rng(3000 + P + 10 * len(name))
    w = net_cases.draw_weights(name, rng)
    c, a = netref.NETS[name]
    wa = w[netref.n_params(c):]
    S = rng.normal(0, 1, (P, 12)).astype(F)
    z = rng.uniform(-1.5, 1.5, (P, 4))
    mean, _ = netref.policy64(a, wa, S, np.zeros((P, 4)))
    A = (mean + STD * z).astype(F)
    _, lp = netref.policy64(a, wa, S, A)
    i, d = np.meshgrid(np.arange(P), np.arange(4), indexing="ij")
    rho = np.array(net_cases.RHO)[(i + d) % 4]
    L = (lp - np.log(rho)).astype(F)
    G = rng.normal(0, 5, P).astype(F)
    sign = np.where((np.arange(P) // 4) % 2 == 0, 1.0, -1.0)
    Ad = (sign * (0.1 + np.abs(rng.normal(0, 1, P)))).astype(F)
    traj = dict(states=S.reshape(T, n, 12), actions=A.reshape(T, n, 4), logp=L.reshape(T, n, 4),
                rewards=G.reshape(T, n), dones=np.ones((T, n), np.uint8),
                values=(G - Ad).astype(F).reshape(T, n))
    for v in traj.values():
        v.setflags(write=False)
    return w, traj


def with_skips(traj, rows, d=2, poison=None):
    """a copy with logp_old[rows, d] = -200 (expf == 0 in fp32).  poison "nan": the rows' states
    and rewards (so returns and advantages) NaN, actions +inf; "inf": rewards -inf against a zero
    old value (returns and advantages -inf), states NaN, actions +inf"""
    T, n = traj["rewards"].shape
    out = {k: v.copy().reshape((T * n,) + v.shape[2:]) for k, v in traj.items()}
    out["logp"][rows, d] = -200.0
    if poison:
        out["states"][rows] = np.nan
        out["actions"][rows] = np.inf
        out["rewards"][rows] = np.nan if poison == "nan" else -np.inf
        if poison == "inf":
            out["values"][rows] = 0.0
    return {k: v.reshape(traj[k].shape) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def forward64(name, P):
    """float64 (lp [P, 4], V [P]) of the case's networks on its rows"""
    w, traj = case(name, P)
    c, a = netref.NETS[name]
    nc = netref.n_params(c)
    S = traj["states"].reshape(P, 12)
    _, lp = netref.policy64(a, w[nc:], S, traj["actions"].reshape(P, 4))
    V, _ = netref._forward64(netref.layers(c), netref.split(c, w[:nc].astype(np.float64)), S.astype(np.float64))
    return lp, V[:, 0]


def counted(logp_old):
    """the skip rule: a row counts unless expf(logp_old) == 0 in fp32 in any dimension"""
    with np.errstate(under="ignore"):
        return ~(np.exp(np.asarray(logp_old, F)) == F(0)).any(axis=1)


def stats64(lp, V, logp_old, ret, adv, eps_clip=EPS_CLIP, fp32_diff=False):
    """every statistic of wk_ppo_stats in float64 from per-row log-densities lp [P, 4] and values
    V [P] (float64, or the kernel's fp32 outputs) and the buffer's fp32 logp_old / returns /
    advantages.  fp32_diff: d = lp - logp_old is the fp32 difference of fp32 values, as the kernel
    forms it, and float64 from there.  Also the sums of |term| and the per-entry ratios the tests'
    bounds need."""
    nan = float("nan")
    use = counted(logp_old)
    n = int(use.sum())
    out = dict(samples=n, skipped=int((~use).sum()))
    d32 = (np.asarray(lp, F) - np.asarray(logp_old, F))[use] if fp32_diff else None
    lp, V = np.asarray(lp, np.float64)[use], np.asarray(V, np.float64)[use]
    L = np.asarray(logp_old, np.float64)[use]
    ret, adv = np.asarray(ret, np.float64)[use], np.asarray(adv, np.float64)[use][:, None]
    d = d32.astype(np.float64) if fp32_diff else lp - L
    r = np.exp(d)
    lo, up = float(F(1) - F(eps_clip)), float(F(1) + F(eps_clip))
    kl_t, sur_t = np.expm1(d) - d, np.minimum(r * adv, np.clip(r, lo, up) * adv)
    e = ret - V
    mean = lambda x: float(np.mean(x)) if n else nan
    out.update(kl=mean(kl_t), kl_k1=mean(-d), clip_fraction=mean((r > up) | (r < lo)),
               clipped=int(((r > up) | (r < lo)).sum()), ratio_max=float(r.max()) if n else nan,
               surrogate=mean(sur_t), value_loss=mean(e * e))
    var_r = float(np.var(ret)) if n else 0.0
    out["explained_variance"] = 1.0 - float(np.var(e)) / var_r if var_r > 0 else nan
    out["abs"] = dict(kl=float(np.abs(kl_t).sum()), kl_k1=float(np.abs(d).sum()),
                      surrogate=float(np.abs(sur_t).sum()), value_loss=float((e * e).sum()))
    out["ratios"], out["d"], out["e"] = r, d, e
    return out
