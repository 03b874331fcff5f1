"""GPU: ReturnsMode = 1 -- k_returns_std (csrc/wk_returns.hip), the bootstrap values and their
calls; and ReturnsMode = 0's k_returns, the same scan's other instantiation, bit for bit.

  * both kernels against the float32 restatement (tests/retref.py), bit for bit, on caller data:
    n in {1, 63, 64, 65, 257} (257 crosses the 256-lane block), T in {1, 2, 64} at Horizon 64,
    Monte-Carlo and GAE, five done patterns; the bootstrap value is in mode 1's last row and not
    in mode 0's;
  * non-finite bootstrap values: nothing passes an episode end, and a NaN stays in its column;
  * NormalizeAdvantages on top (k_normalize, unchanged) at the bar tests/test_gpu_parity.py
    applies to normalised advantages: rtol 1e-5, atol 1e-6; and k_normalize alone from one element
    to 4,160 (below, at and above its 1,024 threads) on standard, offset and constant advantages;
  * rollouts of a built-in and two general contexts across episode ends inside and at the cut:
    the bootstrap values are value(get_obs()) bit for bit, the returns the restatement of the
    fetched rows;
  * end to end: with zero bootstrap values a Monte-Carlo update is the ReturnsMode = 0 update in
    every bit of the weights and Adam's moments; with the critic's values it is another one;
  * the call-order errors (WK_ERR_STATE).
"""
import numpy as np
import pytest

import retref
from test_gpu_net import _engine, _weights

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 20250905
GAMMA, LAMBDA, EPS = 0.9, 0.95, 0.3  # wk_config_defaults
PATTERNS = ["none", "last", "first", "every", "random"]


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _dones(pattern, T, n, g):
    d = np.zeros((T, n), np.uint8)
    if pattern == "last":
        d[T - 1] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern == "every":
        d[:] = 1
    elif pattern == "random":
        d = (g.random((T, n)) < 0.1).astype(np.uint8)
    return d


def _inputs(T, n, g):
    r = g.uniform(-40, 80, (T, n)).astype(F)
    v = (10 * g.standard_normal((T, n))).astype(F)
    vlast = (10 * g.standard_normal(n)).astype(F)
    return r, v, vlast


def _run(eng, r, v, d, vlast, mode=1):
    """set_trajectory + set_bootstrap_values (ReturnsMode 1 only: a mode-0 context has none) +
    compute_returns + get_trajectory"""
    T, n = r.shape
    eng.set_trajectory(np.zeros((T, n, 12), F), np.zeros((T, n, 4), F), np.zeros((T, n, 4), F), r, d, v)
    if mode == 1:
        eng.set_bootstrap_values(vlast)
    eng.compute_returns()
    tr = eng.get_trajectory(T)
    if mode == 1:
        np.testing.assert_array_equal(_bits(eng.get_bootstrap_values()), _bits(vlast))
    return tr["returns"], tr["advantages"]


def _expect_wk_error(wk, code, fn, *a, word=None):
    with pytest.raises(wk.WkError) as ex:
        fn(*a)
    assert f"({code})" in str(ex.value), str(ex.value)
    if word:
        assert word in str(ex.value), str(ex.value)


# both ReturnsMode values: the two kernels are one scan's text (returns_scan<STD>).  The mode-1 cases
# keep the ids they had before the test took a mode ("n-use_gae"); the mode-0 cases add "-mode0".
_BITWISE = [(n, use_gae, mode) for mode in (1, 0) for n in (1, 63, 64, 65, 257) for use_gae in (0, 1)]


@pytest.mark.parametrize("n,use_gae,mode", _BITWISE,
                         ids=[f"{n}-{u}" + ("" if m == 1 else "-mode0") for n, u, m in _BITWISE])
def test_kernel_equals_restatement_bit_for_bit(wk, n, use_gae, mode):
    eng = wk.Engine(n, seed=SEED, Horizon=64, ReturnsMode=mode, UseGAE=use_gae)
    g = np.random.default_rng(1000 * n + use_gae)
    for T in (1, 2, 64):
        for pattern in PATTERNS:
            r, v, vlast = _inputs(T, n, g)
            d = _dones(pattern, T, n, g)
            ret, adv = _run(eng, r, v, d, vlast, mode)
            xret, xadv = retref.returns32(mode, use_gae, GAMMA, LAMBDA, r, v, d, vlast)
            np.testing.assert_array_equal(_bits(ret), _bits(xret), err_msg=f"ret T={T} {pattern}")
            np.testing.assert_array_equal(_bits(adv), _bits(xadv), err_msg=f"adv T={T} {pattern}")
            if pattern == "none" and mode == 1:  # the bootstrap value is in the last row (a step of 0.9)
                other = retref.returns32(1, use_gae, GAMMA, LAMBDA, r, v, d, vlast + F(1))[0]
                assert (other[T - 1] != ret[T - 1]).all()
            elif pattern == "none":  # mode 0 starts from 0: no bootstrap value is in the last row
                other = retref.returns32(1, use_gae, GAMMA, LAMBDA, r, v, d, vlast)[0]
                assert (other[T - 1] != ret[T - 1]).all()
    eng.close()


@pytest.mark.parametrize("use_gae", [0, 1])
def test_nonfinite_bootstrap_values(wk, use_gae):
    n, T = 65, 64
    eng = wk.Engine(n, seed=SEED, Horizon=T, ReturnsMode=1, UseGAE=use_gae)
    g = np.random.default_rng(7 + use_gae)
    r, v, vlast = _inputs(T, n, g)
    # NaN behind an episode end: the done step assigns 0, so nothing of it arrives
    d = _dones("random", T, n, g)
    ended = np.arange(n) % 2 == 0
    d[T - 1] = ended
    vl = np.where(ended, F(np.nan), vlast).astype(F)
    ret, adv = _run(eng, r, v, d, vl)
    xret, xadv = retref.returns32(1, use_gae, GAMMA, LAMBDA, r, v, d, vl)
    assert np.isfinite(ret).all() and np.isfinite(adv).all()
    np.testing.assert_array_equal(_bits(ret), _bits(xret))
    np.testing.assert_array_equal(_bits(adv), _bits(xadv))
    # NaN for one walker that never ends: its column alone is NaN
    d = _dones("none", T, n, g)
    vl = vlast.copy()
    vl[5] = np.nan
    ret, adv = _run(eng, r, v, d, vl)
    xret, xadv = retref.returns32(1, use_gae, GAMMA, LAMBDA, r, v, d, vl)
    keep = np.arange(n) != 5
    for got, ref in ((ret, xret), (adv, xadv)):
        assert np.isnan(got[:, 5]).all() and np.isnan(ref[:, 5]).all()
        np.testing.assert_array_equal(_bits(got[:, keep]), _bits(ref[:, keep]))
        assert np.isfinite(got[:, keep]).all()
    eng.close()


@pytest.mark.parametrize("n,T", retref.NORMALIZE_SIZES)
def test_normalize_sizes_and_kinds(wk, n, T):
    """k_normalize (one block of 1,024 threads striding over n T elements) below, at and above the
    block, on standard, offset (mean 3e4, spread 1: tests/test_retref.py shows float sums miss the
    bar there) and constant advantages.  Every step ends an episode and the values are zero, so the
    advantages are the rewards bit for bit."""
    eng = wk.Engine(n, seed=SEED, Horizon=64, ReturnsMode=1, UseGAE=0, NormalizeAdvantages=1)
    d = np.ones((T, n), np.uint8)
    v = np.zeros((T, n), F)
    for kind in retref.NORMALIZE_KINDS:
        x = retref.normalize_case(kind, n, T)
        ret, adv = _run(eng, x, v, d, np.zeros(n, F))
        xret, xadv = retref.returns32(1, 0, GAMMA, LAMBDA, x, v, d, np.zeros(n, F))
        np.testing.assert_array_equal(_bits(xadv), _bits(x))
        np.testing.assert_array_equal(_bits(ret), _bits(xret), err_msg=kind)
        assert adv.shape == (T, n)
        np.testing.assert_allclose(adv, retref.normalize32(xadv, EPS), rtol=1e-5, atol=1e-6, err_msg=kind)
        if kind == "constant" or n * T == 1:  # (x - mean) is exactly 0, over sd + Epsilon > 0
            assert not adv.any(), kind
        else:
            assert np.isfinite(adv).all() and adv.any(), kind
    eng.close()


def test_normalised_advantages(wk):
    n, T = 65, 64
    eng = wk.Engine(n, seed=SEED, Horizon=T, ReturnsMode=1, UseGAE=1, NormalizeAdvantages=1)
    g = np.random.default_rng(11)
    r, v, vlast = _inputs(T, n, g)
    d = _dones("random", T, n, g)
    ret, adv = _run(eng, r, v, d, vlast)
    xret, xadv = retref.returns32(1, 1, GAMMA, LAMBDA, r, v, d, vlast)
    np.testing.assert_array_equal(_bits(ret), _bits(xret))
    np.testing.assert_allclose(adv, retref.normalize32(xadv, EPS), rtol=1e-5, atol=1e-6)
    eng.close()


@pytest.mark.parametrize("use_gae", [0, 1])
@pytest.mark.parametrize("name", ["builtin", "tiny", "odd"])
def test_rollout_fills_bootstrap_values(wk, name, use_gae):
    """MaxTimesteps = 5: an episode has 6 steps, so the 12-step rollout ends episodes inside and
    at the cut, and the 9-step one that follows is cut mid-episode (T < Horizon)"""
    n = 17
    cfg = dict(Horizon=12, MaxTimesteps=5, RandomizeStart=1, ReturnsMode=1, UseGAE=use_gae)
    if name == "builtin":
        eng = wk.Engine(n, seed=SEED, **cfg)
    else:
        eng = _engine(wk, name, n=n, **cfg)
        eng.set_weights(_weights(name, 3))
    for k, T in enumerate((12, 9)):
        eng.rollout(T)
        vlast = eng.get_bootstrap_values()
        np.testing.assert_array_equal(_bits(vlast), _bits(eng.value(eng.get_obs())))
        tr = eng.get_trajectory(T)
        d = tr["dones"].astype(bool)
        assert d[:T - 1].any(), "no episode ended inside the rollout"
        if k == 0:
            assert d[T - 1].any(), "no episode ended at the cut"
        else:
            assert not d[T - 1].all(), "no episode was cut"
        xret, xadv = retref.returns32(1, use_gae, GAMMA, LAMBDA, tr["rewards"], tr["values"], tr["dones"], vlast)
        np.testing.assert_array_equal(_bits(tr["returns"]), _bits(xret), err_msg=f"rollout {k}")
        np.testing.assert_array_equal(_bits(tr["advantages"]), _bits(xadv), err_msg=f"rollout {k}")
        cut = ~d[T - 1]
        if cut.any():  # the critic's value is in the cut walkers' last return
            zret = retref.returns32(1, use_gae, GAMMA, LAMBDA, tr["rewards"], tr["values"], tr["dones"],
                                    np.zeros(n, F))[0]
            assert not np.array_equal(zret[T - 1][cut], xret[T - 1][cut])
    eng.close()


def test_zero_bootstrap_update_equals_mode_0(wk):
    n, T = 64, 16
    cfg = dict(Horizon=T, Minibatch=256, Epochs=2, RandomizeStart=1)

    def run(mode, zeros):
        eng = wk.Engine(n, seed=SEED, ReturnsMode=mode, **cfg)
        eng.rollout(T)
        if zeros:
            eng.set_bootstrap_values(np.zeros(n, F))
        eng.ppo_update(update_index=0)
        out = (eng.get_weights(), *eng.get_adam())
        eng.close()
        return out

    w0, m0, v0, t0 = run(0, False)
    w1, m1, v1, t1 = run(1, True)
    assert t0 == t1 == 2 * (n * T // 256)
    np.testing.assert_array_equal(_bits(w1), _bits(w0))
    np.testing.assert_array_equal(_bits(m1), _bits(m0))
    np.testing.assert_array_equal(_bits(v1), _bits(v0))
    w2 = run(1, False)[0]  # the critic's values at the cut: another update
    assert np.isfinite(w2).all() and not np.array_equal(w2, w0)


def test_state_errors(wk, tmp_path):
    n, T = 4, 4
    g = np.random.default_rng(3)
    r, v, vlast = _inputs(T, n, g)
    d = _dones("none", T, n, g)
    traj = (np.zeros((T, n, 12), F), np.zeros((T, n, 4), F), np.zeros((T, n, 4), F), r, d, v)
    eng = wk.Engine(n, seed=SEED, Horizon=T, Minibatch=8, ReturnsMode=1)
    _expect_wk_error(wk, -5, eng.get_bootstrap_values)  # nothing recorded yet
    _expect_wk_error(wk, -5, eng.set_bootstrap_values, vlast)
    eng.set_trajectory(*traj)
    for call in (eng.compute_returns, eng.ppo_update, eng.time_gradient, eng.get_bootstrap_values):
        _expect_wk_error(wk, -5, call, word="wk_set_bootstrap_values")
    eng.set_bootstrap_values(vlast)
    eng.compute_returns()
    np.testing.assert_array_equal(_bits(eng.get_trajectory(T)["returns"]),
                                  _bits(retref.returns32(1, 0, GAMMA, LAMBDA, r, v, d, vlast)[0]))
    eng.set_trajectory(*traj)  # a new trajectory: the values left with the old one
    _expect_wk_error(wk, -5, eng.compute_returns, word="wk_set_bootstrap_values")
    eng.rollout(T)
    eng.get_bootstrap_values()
    path = str(tmp_path / "ckpt.bin")
    eng.checkpoint_save(path)
    eng.checkpoint_load(path)
    _expect_wk_error(wk, -5, eng.get_bootstrap_values)
    eng.close()
    ref = wk.Engine(n, seed=SEED, Horizon=T)  # ReturnsMode = 0: both calls are refused
    ref.rollout(T)
    _expect_wk_error(wk, -5, ref.get_bootstrap_values, word="ReturnsMode")
    _expect_wk_error(wk, -5, ref.set_bootstrap_values, vlast, word="ReturnsMode")
    ref.close()
