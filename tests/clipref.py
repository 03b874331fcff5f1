"""Restatement of MaxGradNorm (include/wk_api.h, k_clip_adam in csrc/wk_tail.hip) -- test
infrastructure only (numpy).  Per network (critic = parameters [0, n_critic), actor the rest):

    norm  = sqrt(sum (double)g * (double)g)       g the fp32 summed gradient
    coef  = (double)MaxGradNorm / (norm + 1e-6)   (torch.nn.utils.clip_grad_norm_'s form)
    scale = (float)coef if norm is finite and coef < 1 else 1
    g'    = g * scale                             one fp32 product, then netref.adam32(g')

The order of the sum is not restated: n terms in double differ between two orders by at most
n * 2^-53 relative, which the tests allow for (tests/test_gpu_clip.py).
"""
import numpy as np

import netref

F = np.float32


def norms(g, n_critic):
    """float64 L2 norms (critic, actor) of the flat fp32 gradient"""
    g = np.asarray(g, F).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(np.sum(g[:n_critic] * g[:n_critic]))), float(np.sqrt(np.sum(g[n_critic:] * g[n_critic:])))


def scale_of(norm, max_norm):
    """the fp32 factor of one network: max_norm is wk_config.MaxGradNorm (a float32 value)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        coef = np.float64(F(max_norm)) / (np.float64(norm) + np.float64(1e-6))
    return F(coef) if np.isfinite(norm) and coef < 1.0 else F(1.0)


def scaled_gradient(g, n_critic, scales):
    """g' = g * scale per network (one fp32 product)"""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        return np.concatenate([g[:n_critic] * F(scales[0]), g[n_critic:] * F(scales[1])]).astype(F)


def clip_adam32(w, m, v, g, t, n_critic, max_norm, alpha=1e-3, scales=None):
    """one clipped Adam step (step count t, from 1): returns (w, m, v, norms, scales); `scales`
    replaces the rule's factors (a test that pins them to the engine's reported ones)"""
    nr = norms(g, n_critic)
    sc = tuple(scale_of(x, max_norm) for x in nr) if scales is None else tuple(F(s) for s in scales)
    with np.errstate(invalid="ignore"):
        w2, m2, v2 = netref.adam32(w, m, v, scaled_gradient(g, n_critic, sc), t, alpha=alpha)
    return w2, m2, v2, nr, sc
