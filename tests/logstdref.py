"""float64 restatement of the log-std pass (wk_log_std_gradient, the LearnLogStd = 1 step) on top
of tests/netref.py and tests/statsref.py -- test infrastructure only (numpy).
tests/test_logstdref.py checks it without a GPU; tests/test_gpu_logstd.py uses it.

  * grad64: the derivative of -mean(clipped surrogate) by the scalar log-std s in float64.  It
    forms lp itself from the float64 mean with std = exp(s) unrounded: netref.policy64 rounds std
    to fp32, which is right for values and wrong for a derivative.
  * surrogate64: the float64 mean surrogate as a function of s (the finite difference's subject).
  * consts32 / terms32: the engine's fp32 std and log-density constant of a log-std, and the
    kernel's fp32 formation of w and zz from a row's fp32 lp, logp_old and advantage.  The kernel
    forms zz = ((act - mean) / std)^2 and lp = lp_const - zz / 2; a test sees lp only, so terms32
    recovers zz = 2 (lp_const - lp) in fp32, and zz_bracket gives the interval of every zz whose
    lp rounds to the observed one.
  * adam_scalar: the host's Adam step on the scalar, literally.
  * tight: a statsref case whose actions lie closer to the mean than std says (actions = mean +
    0.3 std z), with logp_old the float64 lp at s (every ratio 1, inside the bounds) and every
    advantage positive (or, negated, negative).
"""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

import netref
import statsref

F = np.float32
EPS_CLIP = statsref.EPS_CLIP
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def bounds(eps_clip=EPS_CLIP):
    """the clip bounds as the engine forms them: 1 -+ Epsilon in fp32"""
    return float(F(1) - F(eps_clip)), float(F(1) + F(eps_clip))


def _select(r, adv, lo, up):
    """w = r (partA + partB partC): the gradient kernels' selection of d surrogate / d lp, in the
    arrays' own precision"""
    cr = np.clip(r, lo, up)
    ra, cra = r * adv, cr * adv
    partA = (ra <= cra) * adv
    partB = (cra < ra) * adv
    partC = (r >= lo) & (r <= up)
    return r * (partA + partB * partC)


def _lp64(mean64, actions, s):
    zz = ((np.asarray(actions, np.float64) - mean64) / math.exp(s)) ** 2
    return -s - LOG_SQRT_2PI - zz / 2.0, zz


def surrogate64(mean64, actions, logp_old, adv, s, eps_clip=EPS_CLIP):
    """float64 mean over the counted entries of min(r adv, clip(r) adv) at log-std s"""
    use = statsref.counted(logp_old)
    lp, _ = _lp64(mean64[use], np.asarray(actions)[use], s)
    r = np.exp(lp - np.asarray(logp_old, np.float64)[use])
    a = np.asarray(adv, np.float64)[use][:, None]
    lo, up = bounds(eps_clip)
    return float(np.mean(np.minimum(r * a, np.clip(r, lo, up) * a)))


def entries64(mean64, actions, logp_old, adv, s, eps_clip=EPS_CLIP):
    """float64 (w, zz, lp) of the counted entries, [rows, 4] each"""
    use = statsref.counted(logp_old)
    lp, zz = _lp64(mean64[use], np.asarray(actions)[use], s)
    r = np.exp(lp - np.asarray(logp_old, np.float64)[use])
    a = np.asarray(adv, np.float64)[use][:, None]
    lo, up = bounds(eps_clip)
    return _select(r, a, lo, up), zz, lp


def grad64(mean64, actions, logp_old, adv, s, eps_clip=EPS_CLIP):
    """(gradient of -mean surrogate by s, sum |term|, the counted entries' terms [rows, 4]) with
    term = w (zz - 1); NaN gradient when no row counts"""
    w, zz, _ = entries64(mean64, actions, logp_old, adv, s, eps_clip)
    term = w * (zz - 1.0)
    n = term.size
    return (-float(term.sum()) / n if n else float("nan")), float(np.abs(term).sum()), term


@functools.lru_cache(maxsize=None)
def _libm():
    try:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (m.expf, m.logf, m.sqrtf):
            f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
        return m
    except (OSError, AttributeError):
        return None


def consts32(s):
    """(std, lp_const) as fp32 values the way the engine's host code forms them: expf(s) and
    -logf(std) - logf(sqrtf(2 pi)), with the C library's functions where they can be loaded"""
    m = _libm()
    if m is None:
        std = F(np.exp(F(s)))
        return std, F(F(-np.log(std)) - np.log(np.sqrt(F(2) * F(np.pi))).astype(F))
    std = F(m.expf(float(F(s))))
    two_pi = F(2) * F(3.14159265358979323846)
    return std, F(F(-F(m.logf(float(std)))) - F(m.logf(float(F(m.sqrtf(float(two_pi)))))))


def terms32(lp, logp_old, adv, lp_const, eps_clip=EPS_CLIP):
    """the kernel's fp32 w and zz of every entry from fp32 lp [P, 4], logp_old [P, 4] and adv [P]:
    rr = expf(lp - logp_old), w = rr (partA + partB partC), zz = 2 (lp_const - lp)"""
    lp, L = np.asarray(lp, F), np.asarray(logp_old, F)
    a = np.asarray(adv, F)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.exp((lp - L).astype(F)).astype(F)
        w = _select(r, a, F(1) - F(eps_clip), F(1) + F(eps_clip)).astype(F)
    zz = (F(2) * (F(lp_const) - lp).astype(F)).astype(F)
    return w, zz


def zz_bracket(lp, lp_const):
    """float64 (low, high): every zz with fl32(lp_const - zz / 2) == lp lies inside -- the real
    interval between the midpoints to lp's fp32 neighbours, widened by one place of lp_const (the
    host's logf and the test's may differ there)"""
    lp = np.asarray(lp, F)
    c = float(F(lp_const))
    slack = float(np.spacing(F(lp_const)))
    up = (lp.astype(np.float64) + np.nextafter(lp, F(np.inf)).astype(np.float64)) / 2.0
    dn = (lp.astype(np.float64) + np.nextafter(lp, F(-np.inf)).astype(np.float64)) / 2.0
    return np.maximum(2.0 * (c - slack - up), 0.0), 2.0 * (c + slack - dn)


def adam_scalar(s, m, v, t, g, lr, beta1, beta2, eps, lo, hi):
    """one step of the host's Adam on the scalar log-std: (s', m', v', t', clamped, stepped).
    s, lo, hi are floats holding fp32 values; everything else is double.  A non-finite g takes no
    step."""
    if not math.isfinite(g):
        return float(s), m, v, t, False, False
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    t += 1
    mh = m / (1.0 - math.pow(beta1, t))
    vh = v / (1.0 - math.pow(beta2, t))
    s1 = F(float(s) - lr * mh / (math.sqrt(vh) + eps))
    sc = min(max(s1, F(lo)), F(hi))
    return float(sc), m, v, t, bool(sc != s1), True


@functools.lru_cache(maxsize=None)
def mean64(name, P):
    """the float64 mean [P, 4] of the case's actor on its rows"""
    w, traj = statsref.case(name, P)
    c, a = netref.NETS[name]
    m, _ = netref.policy64(a, w[netref.n_params(c):], traj["states"].reshape(P, 12), np.zeros((P, 4)))
    return m


@functools.lru_cache(maxsize=None)
def tight(name, P, s=-1.0, negated=False):
    """(weights, set_trajectory arrays) of the statsref case with actions = mean + 0.3 std z,
    logp_old = the float64 lp at s and every advantage positive (negated: negative)"""
    w, base = statsref.case(name, P)
    n, T = statsref.SHAPES[P]
    rng = np.random.default_rng(7000 + P + 10 * len(name))
    mean = mean64(name, P)
    A = (mean + 0.3 * math.exp(s) * rng.uniform(-1.5, 1.5, (P, 4))).astype(F)
    lp, _ = _lp64(mean, A, s)
    G = base["rewards"].reshape(P)
    Ad = np.abs(G - base["values"].reshape(P)).astype(F) * F(-1 if negated else 1)
    traj = dict(base, actions=A.reshape(T, n, 4), logp=lp.astype(F).reshape(T, n, 4),
                values=(G - Ad).astype(F).reshape(T, n))
    for x in traj.values():
        x.setflags(write=False)
    return w, traj
