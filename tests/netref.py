"""General restatement of the reference's networks for any pair of DSL strings -- test
infrastructure only (numpy), the counterpart of tests/ref64.py for NetworkKernels = 1.

  * layers(dsl): PPOAgent.ParseLayers (PPOAgent.cs:106-142) -- ("D", in, out) dense layers and
    ("ReLU" | "LeakyReLU" | "TanH", n, n) activations; the first dense layer reads 12 states.
  * forward32: DenseLayer.FeedForward (DenseLayer.cs:82-98) in fp32 with sequential sums
    (z_j = (sum_k W[j][k] x[k], in order) + b_j), ActivationLayer.cs:39-72.
  * adam32: DenseLayer.Adam (DenseLayer.cs:125-159) in fp32, the bias corrections in double.
  * train_batch_grad64: PPOAgent.Train(Batch) (PPOAgent.cs:218-346) in float64, returning
    (grad, abs_sum, critic_diag, actor_diag, skipped) like ref64.train_batch_grad64.
  * train_batch_grad32: the same code with every array and constant in fp32 -- what a correct
    fp32 evaluation may differ from float64 by; tests/net_cases.py chooses inputs on it.

Parameter layout: the .weights order -- critic dense layers, then the actor's, each W (out x in,
row-major) then b.
"""
import re

import numpy as np

F = np.float32
STATE = 12
CRITIC_DEFAULT = "Input |64| (LeakyReLU) |1| Output"
ACTOR_DEFAULT = "Input |64| (LeakyReLU) |64| (LeakyReLU) |4| (TanH) Output"

# the test networks of tests/test_gpu_net.py (critic, actor)
NETS = {
    "default": (CRITIC_DEFAULT, ACTOR_DEFAULT),
    "tiny": ("Input |1| Output", "Input |4| Output"),
    "odd": ("Input |5| (TanH) (ReLU) |1| Output",
            "Input (TanH) |7| (ReLU) |17| |33| (LeakyReLU) |4| Output"),
    "max": ("Input |128| (LeakyReLU) |128| (ReLU) |128| (TanH) |1| Output",
            "Input |128| (ReLU) |128| (TanH) |128| (LeakyReLU) |4| (TanH) Output"),
}
# the edge networks of tests/test_gpu_net_edges.py: widths next to the kernels' tile edges (out
# against 16; in against 4, 16 and 32), widths 1 to 3, stacked activations, and the pairs in which
# one network alone decides the rows of the activation cache
NETS.update({
    "edge16": ("Input |16| (ReLU) |15| (TanH) |1| Output",
               "Input |15| (LeakyReLU) |16| (ReLU) |17| (TanH) |4| Output"),
    "edge32": ("Input |32| (TanH) |31| (LeakyReLU) |1| Output",
               "Input |31| (TanH) |32| (LeakyReLU) |33| (ReLU) |4| Output"),
    "edge64": ("Input |65| (TanH) |63| (LeakyReLU) |1| Output",
               "Input |63| (LeakyReLU) |64| (TanH) |65| (LeakyReLU) |4| (TanH) Output"),
    "edge128": ("Input |127| (LeakyReLU) |128| (TanH) |1| Output",
                "Input |128| (TanH) |127| (LeakyReLU) |4| Output"),
    "narrow": ("Input |1| (TanH) |1| Output", "Input |1| |2| (TanH) |3| |4| Output"),
    "stacked": ("Input (TanH) (LeakyReLU) |9| (TanH) (TanH) (LeakyReLU) |1| Output",
                "Input (ReLU) |4| Output"),
    "big_critic": (NETS["max"][0], NETS["tiny"][1]),
    "big_actor": (NETS["tiny"][0], NETS["max"][1]),
})
EDGE_NAMES = ["edge16", "edge32", "edge64", "edge128", "narrow", "stacked", "big_critic", "big_actor"]


def layers(dsl):
    assert re.match(r"^Input( \|\d+\|| \((ReLU|TanH|LeakyReLU)\))+ Output$", dsl), dsl
    toks = re.sub(r"[|()]|( Output)|(Input )", "", dsl).split(" ")
    out, width = [], STATE
    for t in toks:
        if t.isdigit():
            out.append(("D", width, int(t)))
            width = int(t)
        else:
            out.append((t, width, width))
    return out


def n_params(dsl):
    return sum(i * o + o for k, i, o in layers(dsl) if k == "D")


def split(dsl, flat):
    """[(W, b)] views of one network's flat parameters"""
    out, at = [], 0
    for k, i, o in layers(dsl):
        if k == "D":
            out.append((flat[at:at + o * i].reshape(o, i), flat[at + o * i:at + o * i + o]))
            at += o * i + o
    assert at == len(flat)
    return out


def _act(kind, z):
    if kind == "ReLU":
        return np.where(z > 0, z, np.where(np.isnan(z), z, z * 0))  # MathF.Max(0, z)
    if kind == "LeakyReLU":
        return np.where(z < 0, z.dtype.type(0.2) * z, z)
    return np.tanh(z)


def _dact(kind, z):
    one = z.dtype.type(1)
    if kind == "ReLU":
        return np.where(z < 0, one * 0, one)
    if kind == "LeakyReLU":
        return np.where(z < 0, z.dtype.type(0.2), one)
    return one - np.tanh(z) * np.tanh(z)


def forward32(dsl, flat, X):
    """fp32 forward of one network on X [B, 12], every dense sum sequential in k"""
    x = np.asarray(X, F)
    P = split(dsl, np.asarray(flat, F))
    d = 0
    for kind, i, o in layers(dsl):
        if kind == "D":
            W, b = P[d]
            d += 1
            acc = np.zeros((x.shape[0], o), F)
            for k in range(i):
                acc = acc + x[:, k:k + 1] * W[None, :, k]
            x = acc + b[None, :]
        else:
            x = _act(kind, x).astype(F)
    return x


def _forward64(L, P, X):
    cache, x, d = [], X, 0
    for kind, i, o in L:
        cache.append(x)
        if kind == "D":
            x = x @ P[d][0].T + P[d][1]
            d += 1
        else:
            x = _act(kind, x)
    return x, cache


def _backward64(L, P, cache, g):
    d = sum(1 for l in L if l[0] == "D")
    G, A = [None] * d, [None] * d
    for (kind, i, o), x in zip(L[::-1], cache[::-1]):
        if kind == "D":
            d -= 1
            G[d] = (g.T @ x, g.sum(0))
            A[d] = (np.abs(g).T @ np.abs(x), np.abs(g).sum(0))
            g = g @ P[d][0]
        else:
            g = g * _dact(kind, x)
    flat = lambda Q: np.concatenate([np.concatenate([np.ravel(w), np.ravel(b)]) for w, b in Q])
    return flat(G), flat(A)


def _train_batch_grad(T, critic, actor, w, S, A, L, G, Ad, b_div, log_std=-1.0, eps_clip=0.3):
    """PPOAgent.Train(Batch) with every array and constant of type T (np.float64 / np.float32)"""
    w = np.asarray(w, T)
    S, A, L = (np.asarray(x, T) for x in (S, A, L))
    G, Ad = np.asarray(G, T), np.asarray(Ad, T)
    b_div, one, two = T(b_div), T(1), T(2)
    nc = n_params(critic)
    Lc, La = layers(critic), layers(actor)
    Pc, Pa = split(critic, w[:nc]), split(actor, w[nc:])
    std = T(np.float32(np.exp(np.float32(log_std))))  # MathF.Exp(-1) in fp32
    lp_const = T(-np.log(np.float32(std)) - np.log(np.sqrt(2 * np.pi)))
    V, cc = _forward64(Lc, Pc, S)
    mean, ca = _forward64(La, Pa, S)
    up, lo = one + T(eps_clip), one - T(eps_clip)
    lp = lp_const - ((A - mean) / std) ** 2 / two
    with np.errstate(over="ignore"):  # (fp32: a skipped sample's ratio is exp(197) = inf)
        r = np.exp(lp - L)
    cr = np.clip(r, lo, up)
    Acol = Ad[:, None]
    partA = (r * Acol <= cr * Acol) * Acol
    partB = (cr * Acol < r * Acol) * Acol
    partC = (r >= lo) & (r <= up)
    l = -(partA + partB * partC)
    eo = np.exp(L)
    use = ~(np.float32(0) == np.exp(np.asarray(L, np.float32))).any(axis=1)  # fp32 underflow
    act = np.exp(lp) * ((A - mean) / std ** 2) * (l / np.where(eo == 0, one, eo)) / b_div
    crit = two * (V - G[:, None]) / b_div
    act[~use] = 0
    crit[~use] = 0
    gc, ac = _backward64(Lc, Pc, cc, crit)
    ga, aa = _backward64(La, Pa, ca, act)
    assert T is np.float64 or all(x.dtype == T for x in (gc, ac, ga, aa, act, crit)), "not all fp32"
    return (np.concatenate([gc, ga]), np.concatenate([ac, aa]), crit.sum(), act.mean(axis=1).sum(),
            int((~use).sum()))


def policy64(actor, w_actor, S, A, log_std=-1.0):
    """float64 (mean, per-dimension log-density of the actions A) of the actor at the states S"""
    La = layers(actor)
    mean, _ = _forward64(La, split(actor, np.asarray(w_actor, np.float64)), np.asarray(S, np.float64))
    std = float(np.float32(np.exp(np.float32(log_std))))
    lp_const = float(-np.log(np.float32(std)) - np.log(np.sqrt(2 * np.pi)))
    return mean, lp_const - ((np.asarray(A, np.float64) - mean) / std) ** 2 / 2.0


def train_batch_grad64(critic, actor, w, S, A, L, G, Ad, b_div, log_std=-1.0, eps_clip=0.3):
    """Returns (grad, abs_sum, critic_diag, actor_diag, skipped) in float64; abs_sum[p] is the
    sum over samples of |contribution to grad[p]|."""
    return _train_batch_grad(np.float64, critic, actor, w, S, A, L, G, Ad, b_div, log_std, eps_clip)


def train_batch_grad32(critic, actor, w, S, A, L, G, Ad, b_div, log_std=-1.0, eps_clip=0.3):
    """the same math with every array and constant in np.float32: what a correct fp32 evaluation
    may differ from float64 by (tests/net_cases.py chooses inputs on it)"""
    return _train_batch_grad(np.float32, critic, actor, w, S, A, L, G, Ad, b_div, log_std, eps_clip)


def adam32(w, m, v, g, t, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """one DenseLayer.Adam step (step count t, from 1) in fp32; returns (w, m, v)"""
    w, m, v, g = (np.asarray(x, F) for x in (w, m, v, g))
    b1, b2 = F(beta1), F(beta2)
    m = (g * (F(1) - b1)) + (m * b1)
    v = (v * b2) + ((g * g) * (F(1) - b2))
    bc1 = F(1.0 - float(b1) ** t)
    bc2 = F(1.0 - float(b2) ** t)
    w = w - (((m / bc1) / (np.sqrt(v / bc2) + F(eps))) * F(alpha))
    return w.astype(F), m.astype(F), v.astype(F)


def xavier32(critic, actor, seed, philox):
    """Matrix.FromXavier per dense layer with the engine's Philox addressing: element k of the
    l-th dense layer (critic first) draws philox(seed, (k, l, 0, 5)); biases zero"""
    out, gl = [], 0
    for dsl in (critic, actor):
        for kind, i, o in layers(dsl):
            if kind != "D":
                continue
            std = np.sqrt(F(2.0) / F(o + i)).astype(F)
            W = np.empty(o * i, F)
            for k in range(o * i):
                x = philox(seed, (k, gl, 0, 5))
                u1 = F(((int(x[0]) >> 5) * 67108864.0 + (int(x[1]) >> 6)) / 9007199254740992.0)
                u2 = F(((int(x[2]) >> 5) * 67108864.0 + (int(x[3]) >> 6)) / 9007199254740992.0)
                if u1 == 0:
                    u1 = F(1)
                z = np.sqrt(F(-2.0) * np.log(u1)).astype(F) * np.sin(F(2.0) * F(np.pi) * u2).astype(F)
                W[k] = std * F(z)
            out += [W, np.zeros(o, F)]
            gl += 1
    return np.concatenate(out)
