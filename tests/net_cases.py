"""Inputs of the general networks' edge tests (tests/test_gpu_net_edges.py) and of the built-in
matrix-core gradient kernels' (tests/test_gpu_grad_edges.py), chosen on the CPU by the reference
alone -- test infrastructure only (numpy).  tests/test_netref.py re-checks every condition below
without a GPU; the GPU tests only use the inputs.

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

# ---- the built-in matrix-core gradient kernels (tests/test_gpu_grad_edges.py) ----
# Surrogate draws of the network `default` at the kernels' occupancy edges: chunks of 16 samples;
# 4 units (waves, pairs) per block on k_ppo_grad_mfma / _ws, 2 teams on _tp<2>, 1 on _tp<1>; at most
# 256 blocks; reduction groups of 16 slabs.  33 = three chunks (a block with an idle unit), 64 / 65
# = one block / a second block with one unit, 1024 / 1025 = 16 / 17 slabs, 4096 / 4097, 8192 / 8193
# and 16384 / 16385 = every unit one chunk / unit 0 alone a second chunk with one live row, on
# tp<1>, tp<2> and ws / mfma.
GRAD_EDGE_BS = (1, 15, 16, 17, 33, 64, 65, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)
# the non-default surrogate parameters: Epsilon = 0.1 at LogStandardDeviation = -0.5, the ratios
# around the narrower clip edges
TIGHT = dict(log_std=-0.5, eps_clip=0.1, rho=(0.85, 0.95, 1.05, 1.15))
TIGHT_BS = (33, 96)
# (B, variant) -> seed, the first of 2000 + B, + 100, ... within half the bar (8193: the first
# candidate holds a pre-activation at zero, restatement at 48.2; the second taken)
GRAD_EDGE_CASES = {
    (1, "default"): 2001, (15, "default"): 2015, (16, "default"): 2016, (17, "default"): 2017,
    (33, "default"): 2033, (64, "default"): 2064, (65, "default"): 2065, (1024, "default"): 3024,
    (1025, "default"): 3025, (4096, "default"): 6096, (4097, "default"): 6097,
    (8192, "default"): 10192, (8193, "default"): 10293, (16384, "default"): 18384,
    (16385, "default"): 18385, (33, "tight"): 2033, (96, "tight"): 2096,
}

# the position sweep: one live row at every kind of slot of B = 16391 (1,025 chunks, the last with
# 7 live rows); the last unit of a pass and the first of the next on tp<1>, tp<2> and ws / mfma
SWEEP_B, SWEEP_SEED = 16391, 2391
SWEEP_POSITIONS = tuple(range(16)) + (16, 32, 48, 64) + tuple(
    16 * k for k in (255, 256, 511, 512, 1023, 1024)) + (16390,)

# the permuted gather: (walkers, rows per walker, Minibatch, Epochs) -> seed of the surrogate draw
# of walkers * rows samples.  Pool 771 (no power of two) in minibatches of 256 = base 0, 256, 512
# in each of two epochs; pool 4120 with one minibatch of 4,097 per epoch = the one-live-row chunk
# through the permutation, under both epochs' keys, the second onto non-zero Adam moments
PERM_UPDATE = 5
PERM_CASES = {(257, 3, 256, 2): 2771, (1030, 4, 4097, 2): 6120}


def perm_trajectory(shape):
    """(weights, set_trajectory arrays [T, n, ...]) of a PERM_CASES entry: states, actions and
    logp_old of the surrogate draw; its returns as the rewards and no episode end, so the Monte
    Carlo returns are discounted sums of them; values that leave advantages of both signs"""
    n, T, _, _ = shape
    w, (S, A, L, G, Ad) = surrogate_draw("default", PERM_CASES[shape], B=n * T)
    traj = dict(states=S.reshape(T, n, 12), actions=A.reshape(T, n, 4), logp=L.reshape(T, n, 4),
                rewards=G.reshape(T, n), dones=np.zeros((T, n), np.uint8),
                values=(G - Ad).reshape(T, n))
    return w, traj


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


def restatement_ratio(name, w, batch, b_div=None, log_std=-1.0, eps_clip=0.3):
    """worst ratio of the fp32 restatement against float64 on these inputs"""
    c, a = netref.NETS[name]
    B = len(batch[3]) if b_div is None else b_div
    g64, asum, _, _, _ = netref.train_batch_grad64(c, a, w, *batch, B, log_std, eps_clip)
    g32, _, _, _, _ = netref.train_batch_grad32(c, a, w, *batch, B, log_std, eps_clip)
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
def surrogate_draw(name, seed, B=SURROGATE_B, log_std=-1.0, rho=RHO):
    """B samples with actions near the float64 mean (|z| <= 1.5) and logp_old placed so that the
    ratio r = rho cycles through the four values of `rho` per (sample, dimension); advantages of
    both signs with |Adv| >= 0.1.  Returns (weights, batch).  (The generator's call order is the
    B = 96 draw's: the defaults reproduce it byte for byte.)"""
    rng = np.random.default_rng(seed)
    w = draw_weights(name, rng)
    c, a = netref.NETS[name]
    wa = w[netref.n_params(c):]
    S = rng.normal(0, 1, (B, 12)).astype(F)
    z = rng.uniform(-1.5, 1.5, (B, 4))
    mean, _ = netref.policy64(a, wa, S, np.zeros((B, 4)), log_std)
    std = float(F(np.exp(F(log_std))))
    A = (mean + std * z).astype(F)
    _, lp = netref.policy64(a, wa, S, A, log_std)  # at the rounded actions
    i, d = np.meshgrid(np.arange(B), np.arange(4), indexing="ij")
    rho = np.array(rho)[(i + d) % 4]
    L = (lp - np.log(rho)).astype(F)
    G = rng.normal(0, 5, B).astype(F)
    sign = np.where((np.arange(B) // 4) % 2 == 0, 1.0, -1.0)
    Ad = (sign * (0.1 + np.abs(rng.normal(0, 1, B)))).astype(F)
    return w, (S, A, L, G, Ad)


def surrogate_cells(name, w, batch, eps_clip=0.3, log_std=-1.0):
    """from the float64 reference: (r [B, 4], counts of the six cells [sign][region], and the
    per-dimension float64 sum of actorLoss written out per cell)"""
    S, A, L, G, Ad = batch
    c, a = netref.NETS[name]
    mean, lp = netref.policy64(a, w[netref.n_params(c):], S, A, log_std)
    L64, A64, Ad64 = L.astype(np.float64), A.astype(np.float64), Ad.astype(np.float64)[:, None]
    r = np.exp(lp - L64)
    lo, up = 1.0 - eps_clip, 1.0 + eps_clip
    region = np.where(r < lo, 0, np.where(r > up, 2, 1))
    pos = np.broadcast_to(Ad64 > 0, r.shape)
    counts = np.array([[int(((region == k) & (pos == s)).sum()) for k in range(3)] for s in (False, True)])
    # the derivative of -min(r Adv, clip(r) Adv) / r: -Adv, except 0 where the clip is active
    clipped = (pos & (region == 2)) | (~pos & (region == 0))
    l = np.where(clipped, 0.0, -np.broadcast_to(Ad64, r.shape))
    std = float(F(np.exp(F(log_std))))
    loss = np.exp(lp) * ((A64 - mean) / std ** 2) * (l / np.exp(L64)) / len(G)
    return r, counts, loss.sum(0)


def surrogate_case(name):
    return surrogate_draw(name, SURROGATE_CASES[name])


def grad_edge_params(variant):
    """(surrogate_draw keywords, reference keywords) of a variant of GRAD_EDGE_CASES"""
    if variant == "default":
        return {}, {}
    return dict(log_std=TIGHT["log_std"], rho=TIGHT["rho"]), \
        dict(log_std=TIGHT["log_std"], eps_clip=TIGHT["eps_clip"])


def grad_edge_draw(B, variant, seed):
    return surrogate_draw("default", seed, B=B, **grad_edge_params(variant)[0])


def grad_edge_case(B, variant="default"):
    """(weights, batch) of a GRAD_EDGE_CASES entry"""
    return grad_edge_draw(B, variant, GRAD_EDGE_CASES[(B, variant)])


# ---- Adam state for the moment checks ----
def adam_state(nparam, seed):
    """non-zero m and v >= 0 of the size a trained network's have"""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 1e-2, nparam).astype(F)
    v = (rng.normal(0, 1e-2, nparam) ** 2).astype(F)
    return m, v


def _table_ratio(key, seed):
    """restatement ratio of a CASES / EXTRA_CASES key (network, B) or a SURROGATE_CASES key"""
    name = key[0] if isinstance(key, tuple) else key
    w, batch = draw(*key, seed) if isinstance(key, tuple) else surrogate_draw(key, seed)
    return restatement_ratio(name, w, batch)


def _grad_edge_ratio(key, seed):
    """restatement ratio of a GRAD_EDGE_CASES key (B, variant)"""
    w, batch = grad_edge_draw(*key, seed)
    return restatement_ratio("default", w, batch, **grad_edge_params(key[1])[1])


def _search(keys, first, ratio=_table_ratio):
    out = {}
    for key in keys:
        tried = []
        for k in range(MAX_SEEDS):
            seed = first(key) + 100 * k
            tried.append(ratio(key, seed))
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
    edge = [(B, "default") for B in GRAD_EDGE_BS] + [(B, "tight") for B in TIGHT_BS]
    print(_search(edge, lambda k: 2000 + k[0], _grad_edge_ratio))
