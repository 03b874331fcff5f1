"""CPU: MaxGradNorm's boundary (include/wk_api.h) -- the field's validation before a device is
touched, its default, its absence from the JSON document, the record's layout in the three
mirrors, the NULL-context errors of the three new entry points, k_clip_adam's code-object
metadata -- and self-checks of the restatement the GPU tests compare against (tests/clipref.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import clipref
from test_csharp_binding import cs_struct_layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.mark.parametrize("value", [-1.0, float("nan"), -1e-30])
def test_create_refuses_bad_max_grad_norm_before_the_device(wk, value):
    lib = wk.load_library()
    cfg = wk.default_config(MaxGradNorm=value)
    h = C.c_void_p()
    rc = lib.wk_create(C.byref(cfg), 0, 8, 1, C.byref(h))
    assert rc == -3 and not h.value  # WK_ERR_CONFIG
    assert "MaxGradNorm" in lib.wk_last_error(None).decode()


def test_default_is_off_and_not_in_the_json_document(wk):
    assert wk.default_config().MaxGradNorm == 0.0
    assert "MaxGradNorm" not in wk.config_to_json()
    assert "MaxGradNorm" not in wk.config_to_json(wk.default_config(MaxGradNorm=0.5))
    # appended after TargetKL: every earlier field keeps its offset
    names = [f[0] for f in wk.WkConfig._fields_]
    assert names[-2:] == ["TargetKL", "MaxGradNorm"]


def test_record_layout(wk):
    g = wk.GradNorms
    assert C.sizeof(g) == 8 + 2 * 8 + 2 * 8 + 3 * 2 * 8 + 2 * 4 + 2 * 4 == 104
    assert [(f[0], getattr(g, f[0]).offset) for f in g._fields_] == [
        ("steps", 0), ("clipped", 8), ("nonfinite", 24), ("norm_last", 40), ("norm_max", 56),
        ("norm_sum", 72), ("scale_last", 88), ("pad", 96)]
    lay, size = cs_struct_layouts()["WkGradNorms"]
    assert size == C.sizeof(g)
    assert [(o, s) for _, o, s in lay] == [(getattr(g, f[0]).offset, getattr(g, f[0]).size) for f in g._fields_]


def test_object_apis_call_the_exports():
    api = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "Api.cs")).read()
    nea = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "csrc", "host", "nea.hpp")).read()
    for call in ("wk_grad_norms_get(ctx, out var g)", "wk_set_learning_rate(ctx, alpha)",
                 "wk_get_learning_rate(ctx, out var a)"):
        assert "Wk." + call in api
    for call in ("wk_grad_norms_get(ctx_, &g)", "wk_set_learning_rate(ctx_, alpha)", "wk_get_learning_rate(ctx_, &a)"):
        assert call in nea


def test_null_context_is_an_argument_error(wk):
    lib = wk.load_library()
    g, a = wk.GradNorms(), C.c_float()
    assert lib.wk_grad_norms_get(None, C.byref(g)) == -1  # WK_ERR_ARG
    assert lib.wk_set_learning_rate(None, 1e-3) == -1
    assert lib.wk_get_learning_rate(None, C.byref(a)) == -1


def test_clip_kernel_has_no_scratch(wk):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    res = kernel_resources(wk.LIB_PATH)
    mine = {k: v for k, v in res.items() if "k_clip_adam" in k}
    assert len(mine) == 1, sorted(mine)
    for k, (scratch, spilled, vgprs) in mine.items():
        print(f"{k}: scratch {scratch} spilled {spilled} vgprs {vgprs}")
        assert scratch == 0 and spilled == 0, (k, scratch, spilled)


# ---- the restatement ----
def _grad(n=1028, nc=71, seed=3):
    return np.random.default_rng(seed).normal(0, 1, n).astype(F), nc


def test_scale_is_one_at_or_below_the_bound():
    g, nc = _grad()
    nr = clipref.norms(g, nc)
    for k in range(2):
        # coef = M / (norm + 1e-6) < 1 exactly when M < norm + 1e-6
        assert clipref.scale_of(nr[k], F(nr[k] * 1.001)) == F(1.0)
        assert clipref.scale_of(nr[k], F(nr[k] * 2)) == F(1.0)
        assert clipref.scale_of(nr[k], F(np.inf)) == F(1.0)
        assert clipref.scale_of(nr[k], F(nr[k] * 0.999)) < F(1.0)
    assert clipref.scale_of(0.0, F(0.5)) == F(1.0)  # a zero gradient: coef = 5e5


@pytest.mark.parametrize("bound", [1e-3, 0.5, 3.0])
def test_clipped_norm_is_at_most_the_bound(bound):
    g, nc = _grad()
    nr = clipref.norms(g, nc)
    sc = tuple(clipref.scale_of(x, bound) for x in nr)
    assert all(s < 1 for s in sc)
    after = clipref.norms(clipref.scaled_gradient(g, nc, sc), nc)
    # (float)coef and each fp32 product round once: 2 * 2^-24 relative on every term
    for k in range(2):
        assert after[k] <= float(F(bound)) * (1 + 2.0 ** -22), (k, after[k], bound)
        assert after[k] >= float(F(bound)) * (1 - 1e-5)  # (1e-6 in the denominator, norms >= 8)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_norm_is_not_scaled(bad):
    g, nc = _grad()
    g = g.copy()
    g[5] = bad
    nr = clipref.norms(g, nc)
    assert not np.isfinite(nr[0]) and np.isfinite(nr[1])
    assert clipref.scale_of(nr[0], 1e-3) == F(1.0) and clipref.scale_of(nr[1], 1e-3) < F(1.0)
    w = np.ones(g.size, F)
    w2, m2, v2, _, sc = clipref.clip_adam32(w, np.zeros_like(w), np.zeros_like(w), g, 1, nc, 1e-3)
    assert sc[0] == F(1.0) and np.isfinite(w2[nc:]).all() and np.isfinite(m2[nc:]).all()
    # the actor's step does not see the critic's bad value
    w3, m3, v3, _, _ = clipref.clip_adam32(w, np.zeros_like(w), np.zeros_like(w), _grad()[0], 1, nc, 1e-3)
    for x, y in ((w2, w3), (m2, m3), (v2, v3)):
        np.testing.assert_array_equal(x[nc:].view(np.uint32), y[nc:].view(np.uint32))


def test_scale_one_is_plain_adam():
    import netref
    g, nc = _grad()
    w = np.random.default_rng(1).normal(0, 1, g.size).astype(F)
    m, v = np.zeros_like(w), np.zeros_like(w)
    a = clipref.clip_adam32(w, m, v, g, 1, nc, np.inf)
    b = netref.adam32(w, m, v, g, 1)
    for x, y in zip(a[:3], b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
