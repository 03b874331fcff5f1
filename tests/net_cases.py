"""Inputs of the general networks' edge tests (tests/test_gpu_net_edges.py), chosen on the CPU by
the reference alone -- test infrastructure only (numpy).  tests/test_netref.py re-checks every
condition below without a GPU; the GPU tests only use the inputs.

Why: the gradient bar |g - g64| <= 1e-5 * sum|t| + 1e-7 * max|g64| prices fp32 summation, not a
ReLU / LeakyReLU pre-activation within fp32 rounding of zero, where fp32 and float64 take
different branches of the derivative.  Whether a draw holds such a sample is a property of the
draw.  So a case's seed is the first of 1000 + B, + 100, + 200, ... (at most MAX_SEEDS tried) at
which a plain fp32 numpy evaluation of the same math (netref.train_batch_grad32) stays within
HALF of the bar; the table holds the result as literals (`python tests/net_cases.py` prints it).
A GPU ratio above 1.0 on such inputs is a finding about the kernel.
"""
import numpy as np

import netref

F = np.float32
BS = (1, 15, 16, 17, 33, 16384, 16385)
MAX_SEEDS = 5
HALF = 0.5

# (network, B) -> seed.  The first candidate 1000 + B but for three, which took the second
# (restatement at the first: edge16 B = 15 0.881, big_actor B = 17 0.649, big_actor B = 16384 1.370).
CASES = {
    ("edge16", 1): 1001, ("edge16", 15): 1115, ("edge16", 16): 1016, ("edge16", 17): 1017,
    ("edge16", 33): 1033, ("edge16", 16384): 17384, ("edge16", 16385): 17385,
    ("edge32", 1): 1001, ("edge32", 15): 1015, ("edge32", 16): 1016, ("edge32", 17): 1017,
    ("edge32", 33): 1033, ("edge32", 16384): 17384, ("edge32", 16385): 17385,
    ("edge64", 1): 1001, ("edge64", 15): 1015, ("edge64", 16): 1016, ("edge64", 17): 1017,
    ("edge64", 33): 1033, ("edge64", 16384): 17384, ("edge64", 16385): 17385,
    ("edge128", 1): 1001, ("edge128", 15): 1015, ("edge128", 16): 1016, ("edge128", 17): 1017,
    ("edge128", 33): 1033, ("edge128", 16384): 17384, ("edge128", 16385): 17385,
    ("narrow", 1): 1001, ("narrow", 15): 1015, ("narrow", 16): 1016, ("narrow", 17): 1017,
    ("narrow", 33): 1033, ("narrow", 16384): 17384, ("narrow", 16385): 17385,
    ("stacked", 1): 1001, ("stacked", 15): 1015, ("stacked", 16): 1016, ("stacked", 17): 1017,
    ("stacked", 33): 1033, ("stacked", 16384): 17384, ("stacked", 16385): 17385,
    ("big_critic", 1): 1001, ("big_critic", 15): 1015, ("big_critic", 16): 1016, ("big_critic", 17): 1017,
    ("big_critic", 33): 1033, ("big_critic", 16384): 17384, ("big_critic", 16385): 17385,
    ("big_actor", 1): 1001, ("big_actor", 15): 1015, ("big_actor", 16): 1016, ("big_actor", 17): 1117,
    ("big_actor", 33): 1033, ("big_actor", 16384): 17484, ("big_actor", 16385): 17385,
}
# the same rule for the cases outside that grid: the reduction-group edge (16 / 17 blocks) and the
# base batches of the skip patterns and the Adam check on `odd`
EXTRA_CASES = {
    ("narrow", 256): 1256, ("narrow", 257): 1257, ("odd", 33): 1033, ("odd", 16385): 17385,
}
# cases for which none of the MAX_SEEDS candidates met the condition (kept in the tables with the
# first candidate, and listed here by name)
NO_SEED = ()

# the surrogate-cell batches: network -> seed (first of 2000, 2100, ...)
SURROGATE_B = 96
RHO = (0.5, 0.9, 1.1, 1.5)
SURROGATE_CASES = {"odd": 2000, "default": 2000}


def seed_of(name, B):
    return CASES[(name, B)] if (name, B) in CASES else EXTRA_CASES[(name, B)]


def draw_weights(name, rng):
    """per dense layer W ~ N(0, 2 / (in + out)) then b ~ N(0, 0.1^2), critic first"""
    w = []
    for dsl in netref.NETS[name]:
        for kind, i, o in netref.layers(dsl):
            if kind == "D":
                w += [rng.normal(0, np.sqrt(2 / (i + o)), (o, i)).astype(F).ravel(),
                      rng.normal(0, 0.1, o).astype(F)]
    return np.concatenate(w)


def draw(name, B, seed):
    """weights and batch from one generator, in the order of tests/test_gpu_net.py::_case (which
    seeds it with B + 7); no skipped sample"""
    rng = np.random.default_rng(seed)
    w = draw_weights(name, rng)
    S = rng.normal(0, 1, (B, 12)).astype(F)
    A = rng.normal(0, 1, (B, 4)).astype(F)
    L = rng.normal(-3, 1, (B, 4)).astype(F)
    G = rng.normal(0, 5, B).astype(F)
    Ad = rng.normal(0, 1, B).astype(F)
    return w, (S, A, L, G, Ad)


def case(name, B):
    return draw(name, B, seed_of(name, B))


def ratios(g, g64, asum):
    """|g - g64| over the project's bound, per parameter"""
    return np.abs(g - g64) / (1e-5 * asum + 1e-7 * np.abs(g64).max())


def restatement_ratio(name, w, batch, b_div=None):
    """worst ratio of the fp32 restatement against float64 on these inputs"""
    c, a = netref.NETS[name]
    B = len(batch[3]) if b_div is None else b_div
    g64, asum, _, _, _ = netref.train_batch_grad64(c, a, w, *batch, B)
    g32, _, _, _, _ = netref.train_batch_grad32(c, a, w, *batch, B)
    return float(ratios(g32, g64, asum).max())


# ---- the skip patterns: rows whose logp_old[i, d] = -200 (exp == 0 in fp32) ----
SKIP_PATTERNS = ("first", "tile", "block1", "all")
# The patterns' base batches are the table's B = 33 and B = 16385 cases; no seed is chosen for
# them.  On all but one the fp32 restatement stays within half the bar as well.  The exception,
# with the restatement's worst ratio: dropping rows 16..31 of `edge16` at B = 33 leaves 17 samples
# whose actor gradient the restatement itself misses (18 parameters above 0.5, no pre-activation
# within 1e-4 of zero: the fp32 error of the mean, times (a - mean) / std^2, in terms that the
# dropped rows no longer outweigh).  The GPU test runs that case at the same bar all the same.
SKIP_ABOVE_HALF = {("edge16", 33, "tile"): 1.515}


def skip_rows(pattern, B):
    """None where the pattern does not exist at B"""
    if pattern == "first":
        return np.array([0])
    if pattern == "tile":
        return np.arange(16, 32) if B >= 32 else None
    if pattern == "block1":  # B = 16385: two tiles per block, block 1 starts at sample 32
        return np.array([32]) if B == 16385 else None
    return np.arange(B)


def with_skips(batch, rows, d=2, poison=False):
    """a copy of the batch with logp_old[rows, d] = -200; poison: the other fields of those rows
    non-finite (the reference never reads a skipped sample)"""
    S, A, L, G, Ad = (x.copy() for x in batch)
    L[rows, d] = -200.0
    if poison:
        S[rows] = np.nan
        A[rows] = np.inf
        G[rows] = np.nan
        Ad[rows] = -np.inf
    return S, A, L, G, Ad


# ---- the surrogate cells: sign(Adv) x {r < 1 - eps, inside, r > 1 + eps} ----
def surrogate_draw(name, seed):
    """B = 96 samples with actions near the float64 mean (|z| <= 1.5) and logp_old placed so that
    the ratio r = rho cycles through RHO per (sample, dimension); advantages of both signs with
    |Adv| >= 0.1.  Returns (weights, batch)."""
    B = SURROGATE_B
    rng = np.random.default_rng(seed)
    w = draw_weights(name, rng)
    c, a = netref.NETS[name]
    wa = w[netref.n_params(c):]
    S = rng.normal(0, 1, (B, 12)).astype(F)
    z = rng.uniform(-1.5, 1.5, (B, 4))
    mean, _ = netref.policy64(a, wa, S, np.zeros((B, 4)))
    std = float(F(np.exp(F(-1.0))))
    A = (mean + std * z).astype(F)
    _, lp = netref.policy64(a, wa, S, A)  # at the rounded actions
    i, d = np.meshgrid(np.arange(B), np.arange(4), indexing="ij")
    rho = np.array(RHO)[(i + d) % 4]
    L = (lp - np.log(rho)).astype(F)
    G = rng.normal(0, 5, B).astype(F)
    sign = np.where((np.arange(B) // 4) % 2 == 0, 1.0, -1.0)
    Ad = (sign * (0.1 + np.abs(rng.normal(0, 1, B)))).astype(F)
    return w, (S, A, L, G, Ad)


def surrogate_cells(name, w, batch, eps_clip=0.3):
    """from the float64 reference: (r [B, 4], counts of the six cells [sign][region], and the
    per-dimension float64 sum of actorLoss written out per cell)"""
    S, A, L, G, Ad = batch
    c, a = netref.NETS[name]
    mean, lp = netref.policy64(a, w[netref.n_params(c):], S, A)
    L64, A64, Ad64 = L.astype(np.float64), A.astype(np.float64), Ad.astype(np.float64)[:, None]
    r = np.exp(lp - L64)
    lo, up = 1.0 - eps_clip, 1.0 + eps_clip
    region = np.where(r < lo, 0, np.where(r > up, 2, 1))
    pos = np.broadcast_to(Ad64 > 0, r.shape)
    counts = np.array([[int(((region == k) & (pos == s)).sum()) for k in range(3)] for s in (False, True)])
    # the derivative of -min(r Adv, clip(r) Adv) / r: -Adv, except 0 where the clip is active
    clipped = (pos & (region == 2)) | (~pos & (region == 0))
    l = np.where(clipped, 0.0, -np.broadcast_to(Ad64, r.shape))
    std = float(F(np.exp(F(-1.0))))
    loss = np.exp(lp) * ((A64 - mean) / std ** 2) * (l / np.exp(L64)) / len(G)
    return r, counts, loss.sum(0)


def surrogate_case(name):
    return surrogate_draw(name, SURROGATE_CASES[name])


# ---- Adam state for the moment checks ----
def adam_state(nparam, seed):
    """non-zero m and v >= 0 of the size a trained network's have"""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 1e-2, nparam).astype(F)
    v = (rng.normal(0, 1e-2, nparam) ** 2).astype(F)
    return m, v


def _search(keys, first):
    out = {}
    for key in keys:
        tried = []
        for k in range(MAX_SEEDS):
            seed = first(key) + 100 * k
            w, batch = (draw(*key, seed) if isinstance(key, tuple) else surrogate_draw(key, seed))
            name = key[0] if isinstance(key, tuple) else key
            tried.append(restatement_ratio(name, w, batch))
            if tried[-1] <= HALF:
                break
        ok = tried[-1] <= HALF
        out[key] = seed if ok else first(key)
        print(f"{key!s:24s} seed {out[key]:6d} {'ok' if ok else 'NO SEED'}  ratios tried: "
              + " ".join(f"{x:.3f}" for x in tried))
    return out


if __name__ == "__main__":
    grid = [(n, B) for n in netref.EDGE_NAMES for B in BS]
    print(_search(grid, lambda k: 1000 + k[1]))
    print(_search(list(EXTRA_CASES), lambda k: 1000 + k[1]))
    print(_search(list(SURROGATE_CASES), lambda k: 2000))
