"""CPU: the float64 restatement of the policy statistics (tests/statsref.py) on inputs whose
answers are known, the conditions that make the GPU tests' exact counts and variance bounds
meaningful (tests/test_gpu_stats.py), TargetKL's validation before a device is touched, and the
new kernels' register files (no scratch, no spills)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import net_cases
import netref
import statsref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ppo-bipedalwalker_amd", "libwk.so")
# (family, network, every P of tests/test_gpu_stats.py)
GPU_CASES = [(fam, name, P)
             for fam, name in (("builtin", "default"), ("general", "default"), ("general", "odd"),
                               ("general", "edge16"))
             for P in statsref.SMALL_P + (statsref.large_p(fam),)]


def _inputs(name, P):
    w, traj = statsref.case(name, P)
    lp, V = statsref.forward64(name, P)
    ret = traj["rewards"].reshape(P)
    adv = (traj["rewards"] - traj["values"]).reshape(P)  # the engine's fp32 subtraction
    return lp, V, traj["logp"].reshape(P, 4), ret, adv


def test_large_p_is_one_row_past_a_grid_pass():
    assert statsref.large_p("builtin") == 32769 and statsref.large_p("general") == 16385
    for P, (n, T) in statsref.SHAPES.items():
        assert n * T == P
    assert statsref.second_block_row("general", 33) == 16 and statsref.second_block_row("general", 16385) == 32
    assert statsref.second_block_row("builtin", 33) is None and statsref.second_block_row("builtin", 32769) == 64


def test_same_policy_has_no_divergence():
    lp, V, L, ret, adv = _inputs("odd", 33)
    s = statsref.stats64(lp, V, lp, ret, adv)  # (float64 logp_old = lp64: d is exactly 0)
    assert s["kl"] == 0 and s["kl_k1"] == 0 and s["clip_fraction"] == 0 and s["ratio_max"] == 1
    assert s["samples"] == 33 and s["skipped"] == 0


@pytest.mark.parametrize("rho", net_cases.RHO)
def test_uniform_ratio(rho):
    lp, V, L, ret, adv = _inputs("default", 33)
    s = statsref.stats64(lp, V, lp - np.log(rho), ret, adv)
    assert s["kl"] == pytest.approx(rho - 1 - np.log(rho), rel=1e-12)
    # logp_old = lp - ln rho makes d = lp - logp_old = ln rho (the ratio is rho), and kl_k1 is the
    # mean of -d: -ln rho, whose expectation under the old policy is the KL as well
    assert s["kl_k1"] == pytest.approx(-np.log(rho), rel=1e-12)
    assert s["ratio_max"] == pytest.approx(rho, rel=1e-12)
    assert s["clip_fraction"] == (1.0 if abs(rho - 1) > 0.3 else 0.0)
    # the surrogate: min(rho A, clip(rho) A) per entry
    a = np.repeat(adv.astype(np.float64), 4)
    cl = min(max(rho, float(F(1) - F(0.3))), float(F(1) + F(0.3)))
    assert s["surrogate"] == pytest.approx(np.minimum(rho * a, cl * a).mean(), rel=1e-12)


def test_perfect_critic():
    lp, V, L, ret, adv = _inputs("odd", 17)
    s = statsref.stats64(lp, V, L, V, adv)
    assert s["explained_variance"] == 1.0 and s["value_loss"] == 0.0
    s = statsref.stats64(lp, np.full_like(V, V.mean()), L, V, adv)  # a constant predicts nothing
    assert s["explained_variance"] == pytest.approx(0.0, abs=1e-12)


def test_skip_rule_and_empty_buffer():
    lp, V, L, ret, adv = _inputs("odd", 33)
    L2 = L.copy()
    L2[[0, 5], 2] = -200.0
    s = statsref.stats64(lp, V, L2, ret, adv)
    keep = np.setdiff1d(np.arange(33), [0, 5])
    t = statsref.stats64(lp[keep], V[keep], L[keep], ret[keep], adv[keep])
    assert (s["samples"], s["skipped"]) == (31, 2) and t["skipped"] == 0
    for k in ("kl", "kl_k1", "clip_fraction", "ratio_max", "surrogate", "value_loss", "explained_variance"):
        assert s[k] == t[k], k
    L2[:, 1] = -200.0
    s = statsref.stats64(lp, V, L2, ret, adv)
    assert s["samples"] == 0 and s["skipped"] == 33
    assert all(np.isnan(s[k]) for k in ("kl", "kl_k1", "clip_fraction", "ratio_max", "surrogate",
                                        "value_loss", "explained_variance"))


@pytest.mark.parametrize("family,name,P", GPU_CASES)
def test_gpu_cases_meet_the_conditions(family, name, P):
    """every float64 ratio at least 1e-3 away from both clip bounds (an fp32 ratio, 1e-5 from it,
    falls on the same side: the clip count is exact); Var(ret) >= 1e-2 mean(ret)^2 (the explained
    variance is not a ratio of rounding errors).  One row has no variance: at P = 1 the GPU test
    asserts the NaN instead."""
    lp, V, L, ret, adv = _inputs(name, P)
    s = statsref.stats64(lp, V, L, ret, adv)
    lo, up = float(F(1) - F(0.3)), float(F(1) + F(0.3))
    assert np.abs(s["ratios"] - lo).min() >= 1e-3 and np.abs(s["ratios"] - up).min() >= 1e-3
    assert 0 < s["clipped"] < 4 * P  # both sides of the clip occur
    if P > 4:
        assert (adv > 0).any() and (adv < 0).any()
    if P > 1:
        r = ret.astype(np.float64)
        assert np.var(r) >= 1e-2 * np.mean(r) ** 2
    # the same with each skip pattern applied: the remaining rows keep a variance
    for pat in statsref.SKIP_PATTERNS[:3]:
        rows = statsref.skip_rows(pat, family, P)
        if rows is not None and P > len(rows) + 1:
            r = np.delete(ret.astype(np.float64), rows)
            assert np.var(r) >= 1e-2 * np.mean(r) ** 2


@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf"), -0.5e-30])
def test_create_refuses_bad_target_kl_before_the_device(wk, value):
    lib = wk.load_library()
    cfg = wk.default_config(TargetKL=value)
    h = C.c_void_p()
    rc = lib.wk_create(C.byref(cfg), 0, 8, 1, C.byref(h))
    assert rc == -3 and not h.value  # WK_ERR_CONFIG
    assert "targetkl" in lib.wk_last_error(None).decode().lower()


def test_target_kl_defaults_to_off(wk):
    assert wk.default_config().TargetKL == 0.0
    assert C.sizeof(wk.PpoStats) == 2 * 8 + 7 * 8 + 2 * 4
    lib = wk.load_library()
    st = wk.PpoStats()
    assert lib.wk_policy_stats(None, C.byref(st), None, None) == -1  # WK_ERR_ARG
    assert lib.wk_update_stats_get(None, C.byref(st)) == -1


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/llvm/bin/clang-offload-bundler"),
                    reason="needs the built libwk.so and the ROCm LLVM tools")
def test_stats_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    mine = {k: v for k, v in res.items() if "k_ppo_stats" in k or "k_net_stats" in k or "k_stats_finish" in k}
    assert len(mine) == 3, sorted(mine)
    for k, (scratch, spilled, vgprs) in mine.items():
        assert scratch == 0 and spilled == 0, (k, scratch, spilled)
    # two waves of k_ppo_stats per SIMD: at most 256 of the 512 registers
    assert [v[2] for k, v in mine.items() if "k_ppo_stats" in k][0] <= 256
