"""GPU: MaxGradNorm (per-network gradient-norm clipping in the Adam step, k_clip_adam in
csrc/wk_tail.hip), its record (wk_grad_norms_get) and wk_set_learning_rate, on the built-in and the
general kernels, against the restatement tests/clipref.py.

Inputs: net_cases.draw(name, B, 3000 + B) with the returns multiplied by RET_SCALE = 100, chosen on
the CPU by the float64 reference alone: there the critic's norm is 6.9 (`odd`) to 73 times the
actor's, and case 1 asserts at least 4 from a MaxGradNorm = +inf run.

Bars.  norm_last against numpy's float64 norm of grads_out: 1e-10 relative (two orders of a sum
of n doubles differ by at most n * 2^-53 <= 7.8e-12 at 70,021 terms, plus the square root's
rounding).  scale_last: bit equality with the rule applied to the reported norm_last (double
divide and conversion are IEEE; no fast-math in the build).  Adam's m and v: bit equality with
clipref fed the returned gradient and the reported scale.  The weights: the Adam bar of
tests/test_gpu_net_edges.py, |dw| <= ulp(w) + 4 * 2^-23 * |step|.  Everything else (the
unclipped gradient and diagnostics against a MaxGradNorm = 0 context, +inf against the off path,
repeats, the host exchange against no exchange): bytes.  Each case prints its figures (pytest -s;
measured values: DESIGN.md "Gradient-norm clipping").
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import clipref
import net_cases
import netref
from test_gpu_net import SEED, _engine

pytestmark = pytest.mark.gpu

F = np.float32
RET_SCALE = 100.0
INF = float("inf")


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _make(wk, name, n=4, **cfg):
    """a context of the family: `builtin` the built-in kernels, else the general ones on NETS[name]"""
    return wk.Engine(n, seed=SEED, **cfg) if name == "builtin" else _engine(wk, name, n=n, **cfg)


def _n_critic(name):
    return netref.n_params(netref.NETS["default" if name == "builtin" else name][0])


@functools.lru_cache(maxsize=None)
def _inputs(name, B):
    """(weights, batch) of a case, drawn once; read-only"""
    w, (S, A, L, G, Ad) = net_cases.draw("default" if name == "builtin" else name, B, 3000 + B)
    batch = (S, A, L, (G * F(RET_SCALE)).astype(F), Ad)
    for x in (w, *batch):
        x.setflags(write=False)
    return w, batch


def _step(eng, w, batch, t0):
    """one train_batch Adam step from (w, adam_state, t0); returns everything the call changed"""
    eng.set_weights(w)
    m0, v0 = net_cases.adam_state(eng.nparam, 40 + t0) if t0 else (np.zeros(eng.nparam, F),) * 2
    eng.set_adam(m0, v0, t0)
    g, cd, ad, sk = eng.train_batch(*batch, apply_adam=True)
    m, v, t = eng.get_adam()
    assert t == t0 + 1
    return dict(g=g, cd=cd, ad=ad, sk=sk, m=m, v=v, t=t, w=eng.get_weights(), m0=m0, v0=v0)


def _check_weights(tag, gw, rw, rm, rv, t, alpha=1e-3):
    """the Adam bar of tests/test_gpu_net_edges.py; returns the count of weights not bit-equal"""
    mh = rm.astype(np.float64) / float(F(1.0 - float(F(0.9)) ** t))
    vh = rv.astype(np.float64) / float(F(1.0 - float(F(0.999)) ** t))
    step = float(F(alpha)) * mh / (np.sqrt(vh) + float(F(1e-8)))
    bound = np.spacing(np.abs(rw)).astype(np.float64) + 4 * 2.0 ** -23 * np.abs(step)
    diff = np.abs(gw.astype(np.float64) - rw)
    unequal = int((_bits(gw) != _bits(rw)).sum())
    print(f"{tag}: {unequal} of {gw.size} weights not bit-equal, worst |dw| / bound = {(diff / bound).max():.3f}")
    assert (diff <= bound).all(), (tag, int(np.argmax(diff / bound)), float((diff / bound).max()))
    return unequal


def _check_record_step(tag, rec, g, nc, max_norm):
    """one step's record against numpy: the norms (1e-10), the scales (bits, from the reported norm)"""
    ref = clipref.norms(g, nc)
    for k in range(2):
        rel = abs(rec["norm_last"][k] - ref[k]) / ref[k]
        want = clipref.scale_of(rec["norm_last"][k], max_norm)
        print(f"{tag} net {k}: norm {rec['norm_last'][k]:.17g} numpy {ref[k]:.17g} rel {rel:.2e}  "
              f"scale {rec['scale_last'][k]!r} rule {float(want)!r}")
        assert rel <= 1e-10, (tag, k, rel)
        assert _bits([rec["scale_last"][k]])[0] == _bits([want])[0], (tag, k, rec["scale_last"][k], float(want))
        assert rec["norm_max"][k] == rec["norm_last"][k] == rec["norm_sum"][k]


# ---- 1. one step, bit level ----
STEP_CASES = [("builtin", 1), ("builtin", 17), ("builtin", 64), ("narrow", 17), ("odd", 17),
              ("edge128", 17), ("max", 17)]


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("name,B", STEP_CASES)
def test_one_step_bit_level(wk, name, B, t0):
    w, batch = _inputs(name, B)
    nc = _n_critic(name)
    off = _step(_make(wk, name), w, batch, t0)
    assert off["sk"] == 0 and np.isfinite(off["g"]).all()
    # the measuring run: +inf scales nothing, and is the off path's bits
    eng = _make(wk, name, MaxGradNorm=INF)
    assert eng.nparam == w.size and eng.nparam_critic == nc
    meas = _step(eng, w, batch, t0)
    rec = eng.grad_norms()
    _check_record_step(f"{name} B {B} t0 {t0} inf", rec, meas["g"], nc, INF)
    assert rec["steps"] == 1 and rec["clipped"] == (0, 0) and rec["nonfinite"] == (0, 0)
    for k in ("g", "m", "v", "w"):
        np.testing.assert_array_equal(_bits(meas[k]), _bits(off[k]), err_msg=k)
    ncrit, nact = rec["norm_last"]
    print(f"{name} B {B}: np {w.size} critic norm / actor norm = {ncrit / nact:.2f}")
    assert ncrit >= 4 * nact
    bounds = {"both": (0.5 * nact, (1, 1)), "critic": (math.sqrt(ncrit * nact), (1, 0)), "none": (2 * ncrit, (0, 0))}
    for what, (bound, clipped) in bounds.items():
        tag = f"{name} B {B} t0 {t0} {what}"
        bound = float(F(bound))
        eng = _make(wk, name, MaxGradNorm=bound)
        got = _step(eng, w, batch, t0)
        rec = eng.grad_norms()
        # the gradient buffer and the diagnostics keep the unclipped values
        np.testing.assert_array_equal(_bits(got["g"]), _bits(off["g"]), err_msg=tag)
        assert _bits([got["cd"], got["ad"]]).tolist() == _bits([off["cd"], off["ad"]]).tolist() and got["sk"] == 0
        _check_record_step(tag, rec, got["g"], nc, bound)
        assert rec["steps"] == 1 and rec["clipped"] == clipped and rec["nonfinite"] == (0, 0), (tag, rec)
        assert tuple(s < 1 for s in rec["scale_last"]) == tuple(bool(c) for c in clipped)
        rw, rm, rv, _, _ = clipref.clip_adam32(w, got["m0"], got["v0"], got["g"], t0 + 1, nc, bound,
                                               scales=rec["scale_last"])
        np.testing.assert_array_equal(_bits(got["m"]), _bits(rm), err_msg=tag)
        np.testing.assert_array_equal(_bits(got["v"]), _bits(rv), err_msg=tag)
        _check_weights(tag, got["w"], rw, rm, rv, t0 + 1)
        if what == "none":
            np.testing.assert_array_equal(_bits(got["w"]), _bits(off["w"]), err_msg=tag)
        else:
            assert (_bits(got["m"]) != _bits(off["m"])).any()


# ---- 2, 3. a whole update ----
UPD = dict(Horizon=4, Minibatch=64, Epochs=2)
UPD_STEPS = 2 * (64 * 4 // 64)
FAMILIES = ["builtin", "odd"]


def _update(wk, name, **cfg):
    """rollout + ppo_update on a fresh context: (weights, m, v, t, record or None, engine)"""
    eng = _make(wk, name, n=64, **UPD, **cfg)
    eng.rollout(4)
    eng.ppo_update(update_index=0, sync=False)
    rec = eng.grad_norms() if cfg.get("MaxGradNorm", 0) > 0 else None
    m, v, t = eng.get_adam()
    return eng.get_weights(), m, v, t, rec, eng


def _same_state(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    assert a[3] == b[3]


@pytest.mark.parametrize("name", FAMILIES)
def test_inf_is_the_off_path_in_an_update(wk, name):
    off = _update(wk, name)
    inf = _update(wk, name, MaxGradNorm=INF)
    _same_state(off, inf)
    rec = inf[4]
    print(f"{name} update, MaxGradNorm inf: {rec}")
    assert off[3] == UPD_STEPS and rec["steps"] == UPD_STEPS
    assert rec["clipped"] == (0, 0) and rec["nonfinite"] == (0, 0) and rec["scale_last"] == (1.0, 1.0)
    for k in range(2):
        assert np.isfinite(rec["norm_last"][k]) and rec["norm_last"][k] > 0
        assert rec["norm_max"][k] >= rec["norm_last"][k] > 0
        assert rec["norm_max"][k] >= rec["norm_sum"][k] / UPD_STEPS > 0
    with pytest.raises(wk.WkError) as ex:  # a MaxGradNorm = 0 context keeps no record
        off[5].grad_norms()
    assert "(-5)" in str(ex.value)


@pytest.mark.parametrize("name", FAMILIES)
def test_clipping_acts_in_the_update_deterministically(wk, name):
    off = _update(wk, name)
    a = _update(wk, name, MaxGradNorm=1e-3)
    b = _update(wk, name, MaxGradNorm=1e-3)
    rec = a[4]
    print(f"{name} update, MaxGradNorm 1e-3: {rec}")
    assert rec["steps"] == UPD_STEPS and rec["clipped"] == (UPD_STEPS, UPD_STEPS) and rec["nonfinite"] == (0, 0)
    assert (_bits(a[0]) != _bits(off[0])).any()
    _same_state(a, b)
    assert a[4] == b[4]
    # the record describes the last call: a gradient-only call clears it
    w, batch = _inputs(name, 17)
    a[5].minibatch_gradient(*batch)
    with pytest.raises(wk.WkError) as ex:
        a[5].grad_norms()
    assert "(-5)" in str(ex.value)


# ---- 4. the matrix-core kernels' weight image ----
def test_clipped_step_keeps_the_weight_image(wk):
    w, batch = _inputs("builtin", 64)
    eng = _make(wk, "builtin", MaxGradNorm=0.5)
    _step(eng, w, batch, 0)
    assert eng.grad_norms()["clipped"] == (1, 1)
    fresh = _make(wk, "builtin")
    fresh.set_weights(eng.get_weights())
    a, b = eng.minibatch_gradient(*batch), fresh.minibatch_gradient(*batch)
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
    assert _bits([a[1], a[2]]).tolist() == _bits([b[1], b[2]]).tolist() and a[3] == b[3]
    assert (_bits(eng.get_weights()) != _bits(w)).any()


# ---- 5. a non-finite gradient ----
@pytest.mark.parametrize("name", FAMILIES)
def test_non_finite_critic_gradient(wk, name):
    w, (S, A, L, G, Ad) = _inputs(name, 17)
    G = G.copy()
    G[3] = np.nan
    nc = _n_critic(name)
    eng = _make(wk, name, MaxGradNorm=0.5)
    got = _step(eng, w, (S, A, L, G, Ad), 0)
    rec = eng.grad_norms()
    print(f"{name} NaN return: {rec}")
    assert np.isnan(got["g"][:nc]).any() and np.isfinite(got["g"][nc:]).all()
    assert rec["steps"] == 1 and rec["nonfinite"] == (1, 0) and rec["clipped"] == (0, 1)
    assert np.isnan(rec["norm_last"][0]) and rec["scale_last"][0] == 1.0
    assert rec["norm_max"][0] == 0.0 and rec["norm_sum"][0] == 0.0  # the NaN touched neither
    # the actor's step is the one its own gradient asks for
    ref_norm = clipref.norms(got["g"], nc)[1]
    assert abs(rec["norm_last"][1] - ref_norm) <= 1e-10 * ref_norm
    assert _bits([rec["scale_last"][1]])[0] == _bits([clipref.scale_of(rec["norm_last"][1], 0.5)])[0]
    rw, rm, rv, _, _ = clipref.clip_adam32(w, got["m0"], got["v0"], got["g"], 1, nc, 0.5, scales=rec["scale_last"])
    np.testing.assert_array_equal(_bits(got["m"][nc:]), _bits(rm[nc:]))
    np.testing.assert_array_equal(_bits(got["v"][nc:]), _bits(rv[nc:]))
    _check_weights(f"{name} NaN return, actor", got["w"][nc:], rw[nc:], rm[nc:], rv[nc:], 1)
    # and the actor's gradient is the one of the same batch without the NaN
    clean = _make(wk, name)
    clean.set_weights(w)
    g_clean = clean.train_batch(*_inputs(name, 17)[1], apply_adam=False)[0]
    np.testing.assert_array_equal(_bits(got["g"][nc:]), _bits(g_clean[nc:]))


# ---- 6. launch accounting ----
@pytest.mark.parametrize("name", FAMILIES)
def test_launch_accounting(wk, name):
    for max_norm, adam in ((0.0, 0), (0.5, UPD_STEPS), (INF, UPD_STEPS)):
        eng = _make(wk, name, n=64, MaxGradNorm=max_norm, **UPD)
        eng.rollout(4)
        eng.profile_enable(2)
        eng.ppo_update(update_index=0)
        p = eng.profile()
        eng.profile_enable(0)
        print(f"{name} MaxGradNorm {max_norm}: reduce {p['reduce_launches']} x {p['reduce_ms'] / UPD_STEPS * 1e3:.1f} us, "
              f"adam {p['adam_launches']} launches, {p['adam_ms'] * 1e3:.1f} us in all")
        assert p["grad_launches"] == UPD_STEPS and p["reduce_launches"] == UPD_STEPS
        assert p["adam_launches"] == adam and p["allreduce_calls"] == 0


# ---- 7. exchanges ----
def test_host_exchange_clips_like_no_exchange(wk):
    plain = _update(wk, "builtin", MaxGradNorm=0.5)
    eng = _make(wk, "builtin", n=64, MaxGradNorm=0.5, **UPD)
    calls = []
    eng.comm_init_host(0, 1, lambda buf: calls.append(buf.size))
    eng.rollout(4)
    eng.ppo_update(update_index=0, sync=False)
    rec = eng.grad_norms()
    m, v, t = eng.get_adam()
    _same_state(plain, (eng.get_weights(), m, v, t))
    assert rec == plain[4] and len(calls) == UPD_STEPS
    assert rec["clipped"][0] + rec["clipped"][1] > 0


def test_ipc_exchange_refuses_a_clipping_context(wk):
    eng = _make(wk, "builtin", MaxGradNorm=0.5)
    h = (C.c_uint8 * wk.IPC_HANDLE_BYTES)()
    assert eng.lib.wk_comm_ipc_handle(eng.h, h) == -3  # WK_ERR_CONFIG
    assert "MaxGradNorm" in eng.lib.wk_last_error(eng.h).decode()
    assert eng.lib.wk_comm_init_ipc(eng.h, 0, 1, h) == -3
    assert "MaxGradNorm" in eng.lib.wk_last_error(eng.h).decode()
    assert eng.comm_info()[0] == "none"
    off = _make(wk, "builtin")
    assert len(off.comm_ipc_handle()) == wk.IPC_HANDLE_BYTES  # as before


# ---- 8. the learning rate ----
@pytest.mark.parametrize("name,max_norm", [("builtin", 0.0), ("builtin", 0.5), ("odd", 0.0), ("odd", 0.5)])
def test_set_learning_rate(wk, name, max_norm):
    w, batch = _inputs(name, 17)
    nc = _n_critic(name)
    eng = _make(wk, name, MaxGradNorm=max_norm)
    assert eng.get_learning_rate() == float(F(1e-3))

    def scales():
        return eng.grad_norms()["scale_last"] if max_norm > 0 else (1.0, 1.0)

    eng.set_learning_rate(0.0)
    assert eng.get_learning_rate() == 0.0
    got = _step(eng, w, batch, 0)
    np.testing.assert_array_equal(_bits(got["w"]), _bits(w))
    _, rm, rv, _, _ = clipref.clip_adam32(w, got["m0"], got["v0"], got["g"], 1, nc, max_norm, alpha=0.0, scales=scales())
    np.testing.assert_array_equal(_bits(got["m"]), _bits(rm))
    np.testing.assert_array_equal(_bits(got["v"]), _bits(rv))
    assert rm.any() and rv.any()
    # back to 1e-3: the next step continues from those moments
    eng.set_learning_rate(1e-3)
    for bad in (-1e-3, float("nan"), INF, -INF):
        assert eng.lib.wk_set_learning_rate(eng.h, bad) == -1  # WK_ERR_ARG
        assert eng.get_learning_rate() == float(F(1e-3))
    g2, _, _, _ = eng.train_batch(*batch, apply_adam=True)
    m2, v2, t2 = eng.get_adam()
    assert t2 == 2
    rw, rm2, rv2, _, _ = clipref.clip_adam32(w, rm, rv, g2, 2, nc, max_norm, scales=scales())
    np.testing.assert_array_equal(_bits(m2), _bits(rm2))
    np.testing.assert_array_equal(_bits(v2), _bits(rv2))
    _check_weights(f"{name} MaxGradNorm {max_norm} lr 0 -> 1e-3", eng.get_weights(), rw, rm2, rv2, 2)
    assert (_bits(eng.get_weights()) != _bits(w)).any()
