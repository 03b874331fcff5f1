"""GPU: reward normalisation (wk_reward_norm_*, csrc/wk_rnorm.hip) against tests/rnormref.py
(checked without a GPU by tests/test_rnormref.py).  Crafted trajectories go in through
wk_set_trajectory followed by wk_reward_norm_update; every case prints its figures (pytest -s).

Shapes: n_env in {1, 63, 65, 257} -- below and above a wave and the 256-walker tile, none a
multiple of 4, so the apply kernel's scalar tail runs (T n odd) as well as its float4 body -- and
T in {1, 2, 64} at Horizon 64 (the scan's eight-row batches and its row-by-row tail).

Bars.  acc and the scaled rewards: bit for bit (the latter from the engine's own reported scale).
count, nonfinite, clipped, rows: exact.  mean and m2: |mean - mean*| <= 2 N 2^-53 sum|x| / N and
|m2 - m2*| <= 2 N 2^-53 sum x^2, N the samples so far -- the bound of a sum in any order, the
factor 2 for the merge's few roundings (rnormref.Running.bounds).  scale: within one fp32 ulp of
the formula on the engine's own count, m2 and epsilon; var == m2 / count exactly."""
import struct

import numpy as np
import pytest

import rnormref
from test_gpu_net import _engine as _general_engine

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 20250905
GAMMA = 0.9  # wk_config_defaults
CLIP = 0.25  # bites: raw rewards of tens against a scale of a hundredth


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _same(a, b, msg=""):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    np.testing.assert_array_equal(nan, np.isnan(b), err_msg=msg)
    np.testing.assert_array_equal(_bits(np.where(nan, F(0), a)), _bits(np.where(nan, F(0), b)), err_msg=msg)


def _put(eng, r, d, v=None):
    T, n = r.shape
    v = np.zeros((T, n), F) if v is None else v
    eng.set_trajectory(np.zeros((T, n, 12), F), np.zeros((T, n, 4), F), np.zeros((T, n, 4), F), r, d, v)


def _rec_bytes(s):
    return (int(s["count"]), np.float64(s["mean"]).tobytes(), np.float64(s["m2"]).tobytes(),
            np.float64(s["var"]).tobytes(), F(s["scale"]).tobytes())


def _check_record(s, ref, label):
    """the engine's record against the reference's running state"""
    bm, b2 = ref.bounds()
    print(f"{label}: count {s['count']} nonfinite {s['nonfinite']} mean {s['mean']!r} (ref {ref.mean!r}, "
          f"|d| {abs(s['mean'] - ref.mean):.3e} <= {bm:.3e}) m2 {s['m2']!r} (ref {ref.m2!r}, "
          f"|d| {abs(s['m2'] - ref.m2):.3e} <= {b2:.3e}) scale {s['scale']!r} (ref {float(ref.scale)!r}) "
          f"clipped {s['clipped']}")
    assert s["count"] == ref.count and s["nonfinite"] == ref.nonfinite, label
    assert abs(s["mean"] - ref.mean) <= bm, label
    assert abs(s["m2"] - ref.m2) <= b2, label
    # the scale from the engine's own record
    var, scale = rnormref.scale_of(s["count"], s["m2"], s["epsilon"])
    assert s["var"] == var, label
    assert abs(float(F(s["scale"])) - float(scale)) <= float(np.spacing(scale)), (label, s["scale"], scale)


def _expect(wk, code, fn, *a, word=None):
    with pytest.raises(wk.WkError) as ex:
        fn(*a)
    assert f"({code})" in str(ex.value), str(ex.value)
    if word:
        assert word in str(ex.value), str(ex.value)


def _rewards(g, T, n, special):
    r = g.uniform(-40, 80, (T, n)).astype(F)
    if special:  # NaN and both infinities, each on about 2 % of the rows
        k = g.random((T, n))
        r[k < 0.02] = np.nan
        r[(k >= 0.02) & (k < 0.04)] = np.inf
        r[(k >= 0.04) & (k < 0.06)] = -np.inf
    return r


def _dones(pattern, T, n, g):
    d = np.zeros((T, n), np.uint8)
    if pattern == "last":
        d[T - 1] = 1
    elif pattern == "pairs":  # consecutive dones
        d[::3] = 1
        d[1::3] = 1
    elif pattern == "random":
        d = (g.random((T, n)) < 0.1).astype(np.uint8)
    return d


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_passes_equal_the_restatement(wk, n):
    """acc, the statistics, the scale and the scaled rewards over a sequence of passes on one
    context: every pass after the first exercises the merge and the carry"""
    eng = wk.Engine(n, seed=SEED, Horizon=64)
    eng.reward_norm(clip=CLIP)
    ref = rnormref.Running(n, GAMMA, clip=CLIP)
    g = np.random.default_rng(4000 + n)
    assert eng.reward_norm_state()["scale"] == 1.0 and not eng.reward_acc().any()
    step = 0
    for T in (64, 1, 2, 64):
        for pattern in ("none", "last", "pairs", "random"):
            special = pattern in ("pairs", "random")
            r, d = _rewards(g, T, n, special), _dones(pattern, T, n, g)
            if step == 3:  # a starting acc the host sets
                a0 = g.uniform(-100, 100, n).astype(F)
                eng.set_reward_acc(a0)
                ref.acc = a0.copy()
                _same(eng.reward_acc(), a0)
            before = eng.reward_norm_state()
            _put(eng, r, d)
            # set_trajectory: the apply step alone, with the scale as it is; nothing learned
            s = eng.reward_norm_state()
            assert _rec_bytes(s) == _rec_bytes(before) and s["rows"] == T * n and s["nonfinite"] == 0
            y, clipped = rnormref.apply(r, F(s["scale"]), CLIP)
            _same(eng.scaled_rewards(), y, f"apply-only T={T} {pattern}")
            assert s["clipped"] == clipped
            _same(eng.reward_acc(), ref.acc)
            # the full pass
            eng.reward_norm_update()
            ref.update(r, d)
            s = eng.reward_norm_state()
            label = f"n={n} T={T} {pattern}"
            _same(eng.reward_acc(), ref.acc, label)
            _check_record(s, ref, label)
            y, clipped = rnormref.apply(r, F(s["scale"]), CLIP)
            _same(eng.scaled_rewards(), y, label)
            assert s["clipped"] == clipped and s["rows"] == T * n, label
            assert (s["clip"], s["enabled"], s["frozen"]) == (CLIP, 1, 0)
            if special:
                raw = np.isnan(r)
                assert np.isnan(y[raw]).all() and (y[np.isposinf(r)] == F(CLIP)).all() and (y[np.isneginf(r)] == F(-CLIP)).all()
                assert s["nonfinite"] > 0 or not (~np.isfinite(r)).any()
            assert clipped > 0 or T * n < 63, label  # the clip bites
            _same(eng.get_trajectory(T)["rewards"], r, label)  # the raw rewards stay
            step += 1
    # frozen: the apply step alone from here on
    eng.reward_norm(clip=CLIP, frozen=True)
    before, acc = eng.reward_norm_state(), eng.reward_acc()
    r, d = _rewards(g, 2, n, False), _dones("none", 2, n, g)
    _put(eng, r, d)
    eng.reward_norm_update()
    s = eng.reward_norm_state()
    assert _rec_bytes(s) == _rec_bytes(before) and s["frozen"] == 1
    _same(eng.reward_acc(), acc)
    _same(eng.scaled_rewards(), rnormref.apply(r, F(s["scale"]), CLIP)[0])
    eng.close()


def test_set_state_forms_the_scale(wk):
    eng = wk.Engine(5, seed=SEED, Horizon=4)
    eng.reward_norm(clip=np.inf, epsilon=0.0)
    for count, mean, m2 in ((4, 1.5, 16.0), (1000, -3.0, 123456.789), (0, 0.0, 0.0), (7, 0.0, 0.0)):
        eng.set_reward_norm_state(count, mean, m2)
        s = eng.reward_norm_state()
        var, scale = rnormref.scale_of(count, m2, 0.0)
        assert (s["count"], s["mean"], s["m2"], s["var"]) == (count, mean, m2, var)
        assert abs(s["scale"] - float(scale)) <= float(np.spacing(scale)), (s, scale)
    assert s["scale"] == 1.0  # a zero variance with epsilon 0: not finite, so 1
    eng.close()


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("use_gae", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_returns_read_the_scaled_rewards(wk, mode, use_gae, normalize):
    """the plumbing, with the existing kernels as the yardstick: an enabled context's returns and
    advantages are those of a context never enabled that was fed scaled_rewards()"""
    n, T = 65, 8
    cfg = dict(seed=SEED, Horizon=T, ReturnsMode=mode, UseGAE=use_gae, NormalizeAdvantages=normalize)
    g = np.random.default_rng(77 + 4 * mode + 2 * use_gae + normalize)
    r, d = _rewards(g, T, n, False), _dones("random", T, n, g)
    v = (10 * g.standard_normal((T, n))).astype(F)
    vlast = (10 * g.standard_normal(n)).astype(F)
    a, b = wk.Engine(n, **cfg), wk.Engine(n, **cfg)
    a.reward_norm(clip=CLIP)
    _put(a, r, d, v)
    a.reward_norm_update()
    scaled = a.scaled_rewards()
    assert not np.array_equal(_bits(scaled), _bits(r))
    _put(b, scaled, d, v)
    for e in (a, b):
        if mode == 1:
            e.set_bootstrap_values(vlast)
        e.compute_returns()
    ta, tb = a.get_trajectory(T), b.get_trajectory(T)
    _same(ta["returns"], tb["returns"])
    _same(ta["advantages"], tb["advantages"])
    _same(ta["rewards"], r)
    _same(tb["rewards"], scaled)
    # switched off again the returns read the raw rewards: the context never enabled, fed r
    a.reward_norm(enable=False)
    a.compute_returns()
    _put(b, r, d, v)
    if mode == 1:
        b.set_bootstrap_values(vlast)
    b.compute_returns()
    _same(a.get_trajectory(T)["returns"], b.get_trajectory(T)["returns"])
    a.close()
    b.close()


def test_neutral_setting_changes_no_bit(wk):
    """enabled and frozen with no samples (scale 1) and no clamp: rollout and update are those of
    a context never enabled"""
    n, T = 64, 64
    out = []
    for enable in (False, True):
        eng = wk.Engine(n, seed=SEED, Horizon=T, Minibatch=256, Epochs=2)
        if enable:
            eng.reward_norm(clip=np.inf, frozen=True)
        eng.rollout()
        eng.ppo_update(update_index=0)
        m, v, t = eng.get_adam()
        tr = eng.get_trajectory(T)
        ep, dropped = eng.drain_episodes()
        assert dropped == 0
        out.append((eng.get_weights(), m, v, t, tr["returns"], tr["advantages"], tr["rewards"], ep))
        if enable:
            s = eng.reward_norm_state()
            assert (s["count"], s["scale"], s["rows"], s["clipped"]) == (0, 1.0, n * T, 0)
            _same(eng.scaled_rewards(), tr["rewards"])
            assert not eng.reward_acc().any()
        eng.close()
    p, q = out
    for x, y in zip(p[:3] + p[4:7], q[:3] + q[4:7]):
        _same(x, y)
    assert p[3] == q[3] and p[3] > 0
    assert np.asarray(p[7]).tobytes() == np.asarray(q[7]).tobytes()


def _rollout_engine(wk, family, lanes, n, T):
    if family == "general":
        return _general_engine(wk, "default", n, Horizon=T, LanesPerWalker=lanes)
    return wk.Engine(n, seed=SEED, Horizon=T, LanesPerWalker=lanes)


def _two_rollouts(wk, family, lanes, n=257, T=8):
    """two rollouts on an enabled context, each checked against the restatement run on
    get_trajectory()'s rewards and dones; returns the bytes they left and the rows they came from"""
    eng = _rollout_engine(wk, family, lanes, n, T)
    eng.reward_norm(clip=CLIP)
    ref = rnormref.Running(n, GAMMA, clip=CLIP)
    got, rows = [], []
    for k in range(2):  # the second continues acc and the statistics
        eng.rollout()
        tr = eng.get_trajectory(T)
        ref.update(tr["rewards"], tr["dones"])
        s, acc, y = eng.reward_norm_state(), eng.reward_acc(), eng.scaled_rewards()
        label = f"{family} lanes {lanes} rollout {k}"
        _check_record(s, ref, label)
        _same(acc, ref.acc, label)
        _same(y, rnormref.apply(tr["rewards"], F(s["scale"]), CLIP)[0], label)
        assert s["count"] == (k + 1) * n * T and s["rows"] == n * T
        # the returns are those of the scaled rewards: Monte-Carlo, ReturnsMode 0
        disc = np.zeros(n, F)
        for t in range(T - 1, -1, -1):
            disc = np.where(tr["dones"][t] != 0, F(0), disc)
            disc = (y[t] + (disc * F(GAMMA)).astype(F)).astype(F)
            _same(tr["returns"][t], disc, label)
        got.append((_rec_bytes(s), acc.tobytes(), y.tobytes()))
        rows.append((tr["rewards"], tr["dones"]))
    # reset(mask) zeroes exactly the masked walkers' acc
    a0 = np.arange(1, n + 1, dtype=F)
    eng.set_reward_acc(a0)
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    eng.reset(mask)
    _same(eng.reward_acc(), np.where(mask != 0, F(0), a0))
    eng.reset()
    assert not eng.reward_acc().any()
    assert eng.reward_norm_state()["count"] == 2 * n * T  # the statistics stay
    eng.close()
    return got, rows


def _fed(wk, family, lanes, rows, n=257, T=8):
    """the bytes a context of this mapping leaves when it is fed those rows"""
    eng = _rollout_engine(wk, family, lanes, n, T)
    eng.reward_norm(clip=CLIP)
    got = []
    for r, d in rows:
        _put(eng, r, d)
        eng.reward_norm_update()
        got.append((_rec_bytes(eng.reward_norm_state()), eng.reward_acc().tobytes(), eng.scaled_rewards().tobytes()))
    eng.close()
    return got


def test_real_rollouts_builtin(wk):
    """one-lane and pair mapping, each against the restatement on its own rollouts.  The mappings'
    rollouts themselves differ in the sampled actions' last bits (tests/test_gpu_parity.py holds
    their policies to the oracle at 1e-5), so `the same bytes on every mapping` is asked of the
    same rows: what the one-lane context recorded, fed to a context of every mapping."""
    one, rows = _two_rollouts(wk, "builtin", 1)
    pair, pair_rows = _two_rollouts(wk, "builtin", 2)
    for lanes in (1, 2, 4):
        assert _fed(wk, "builtin", lanes, rows) == one, lanes
    assert _fed(wk, "builtin", 1, pair_rows) == pair
    again, rows2 = _two_rollouts(wk, "builtin", 1)  # and on a repeat
    assert again == one and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(rows, rows2))


def test_real_rollouts_general(wk):
    one, rows = _two_rollouts(wk, "general", 1)
    assert _two_rollouts(wk, "general", 1)[0] == one
    assert _fed(wk, "general", 2, rows) == one


def _version(path):
    with open(path, "rb") as f:
        return struct.unpack("<I", f.read(8)[4:])[0]


def _size(path):
    with open(path, "rb") as f:
        return len(f.read())


def test_snapshot_and_checkpoint(wk, tmp_path):
    n, T = 65, 8
    eng = wk.Engine(n, seed=SEED, Horizon=T)
    eng.reward_norm(clip=CLIP, epsilon=1e-6)
    eng.rollout()
    eng.snapshot()
    s1, a1 = eng.reward_norm_state(), eng.reward_acc()
    eng.rollout()
    assert _rec_bytes(eng.reward_norm_state()) != _rec_bytes(s1) and eng.reward_acc().tobytes() != a1.tobytes()
    eng.restore()
    s, a = eng.reward_norm_state(), eng.reward_acc()
    assert _rec_bytes(s) == _rec_bytes(s1) and a.tobytes() == a1.tobytes() and s["scale"] == s1["scale"]
    # checkpoint round trip into a fresh enabled context, then the same next rollout
    ck, plain_a, plain_b = (str(tmp_path / f) for f in ("rn.ckpt", "a.ckpt", "b.ckpt"))
    eng.checkpoint_save(ck)
    assert _version(ck) == 7
    fresh = wk.Engine(n, seed=SEED, Horizon=T)
    fresh.reward_norm()  # (the file's clip and epsilon replace these)
    fresh.checkpoint_load(ck)
    s = fresh.reward_norm_state()
    assert _rec_bytes(s) == _rec_bytes(s1) and fresh.reward_acc().tobytes() == a1.tobytes()
    assert (s["clip"], s["epsilon"], s["enabled"], s["frozen"]) == (s1["clip"], s1["epsilon"], 1, 0)
    for e in (eng, fresh):
        e.rollout()
    assert eng.scaled_rewards().tobytes() == fresh.scaled_rewards().tobytes()
    assert _rec_bytes(eng.reward_norm_state()) == _rec_bytes(fresh.reward_norm_state())
    assert eng.reward_acc().tobytes() == fresh.reward_acc().tobytes()
    assert eng.get_trajectory(T)["returns"].tobytes() == fresh.get_trajectory(T)["returns"].tobytes()
    # contexts never enabled: version 4, the same size, without the section
    pa, pb = wk.Engine(n, seed=SEED, Horizon=T), wk.Engine(n, seed=SEED, Horizon=T)
    pb.rollout()
    pa.checkpoint_save(plain_a)
    pb.checkpoint_save(plain_b)
    assert _version(plain_a) == _version(plain_b) == 4
    assert _size(plain_a) == _size(plain_b) == _size(ck) - 48 - 4 * n
    # a context never enabled refuses the version-7 file, an enabled one a version-4 file
    _expect(wk, -1, pa.checkpoint_load, ck, word="enable")
    _expect(wk, -1, fresh.checkpoint_load, plain_a, word="version 7")
    assert _rec_bytes(fresh.reward_norm_state()) == _rec_bytes(eng.reward_norm_state())
    pa.checkpoint_load(plain_b)  # and both still work
    # a context enabled and switched off again writes version 4 once more
    fresh.reward_norm(enable=False)
    fresh.checkpoint_save(plain_a)
    assert _version(plain_a) == 4 and _size(plain_a) == _size(plain_b)
    for e in (eng, fresh, pa, pb):
        e.close()


def test_snapshot_before_the_first_enable(wk):
    """a snapshot taken before reward normalisation is first enabled holds none of its state: the
    restore succeeds, puts the walkers back and leaves the record and the running returns alone"""
    n, T = 5, 4
    eng = wk.Engine(n, seed=SEED, Horizon=T)
    eng.snapshot()
    st0 = eng.get_state()
    eng.reward_norm(clip=CLIP)
    eng.rollout()
    s1, a1 = eng.reward_norm_state(), eng.reward_acc()
    assert s1["count"] == n * T and a1.any() and eng.get_state().tobytes() != st0.tobytes()
    eng.restore()
    assert eng.get_state().tobytes() == st0.tobytes()
    assert eng.reward_norm_state() == s1 and _rec_bytes(eng.reward_norm_state()) == _rec_bytes(s1)
    assert eng.reward_acc().tobytes() == a1.tobytes()
    eng.close()


def test_refusals(wk):
    n, T = 5, 4
    on, off, comm = (wk.Engine(n, seed=SEED, Horizon=T) for _ in range(3))
    on.reward_norm()
    # one GPU: the four initialisers on an enabled context
    _expect(wk, -3, on.comm_init_host, 0, 1, lambda buf: None, word="reward normalisation")
    _expect(wk, -3, on.comm_init, 0, 1, bytes(128))
    _expect(wk, -3, on.comm_ipc_handle)
    _expect(wk, -3, on.comm_init_ipc_records, 0, 1, [bytes(wk.IPC_HANDLE_BYTES)])
    comm.comm_init_host(0, 1, lambda buf: None)
    _expect(wk, -3, comm.reward_norm)
    assert comm.reward_norm_state()["enabled"] == 0
    comm.reward_norm(enable=False, clip=3.0)  # (not enabling is no error)
    # never enabled: the state calls are call-order errors, the record is zeros with scale 1
    z = np.zeros(n, F)
    for fn, a in ((off.set_reward_norm_state, (1, 0.0, 1.0)), (off.reward_acc, ()), (off.set_reward_acc, (z,)),
                  (off.reward_norm_update, ()), (off.scaled_rewards, (T,))):
        _expect(wk, -5, fn, *a, word="never enabled")
    s = off.reward_norm_state()
    assert s.pop("scale") == 1.0 and not any(s.values())
    # enabled, without a trajectory
    _expect(wk, -5, on.reward_norm_update)
    _expect(wk, -5, on.scaled_rewards, T)
    # bad arguments change nothing
    on.set_reward_norm_state(10, 2.0, 40.0)
    before = on.reward_norm_state()
    for kw in (dict(clip=0.0), dict(clip=-1.0), dict(clip=np.nan), dict(epsilon=-1e-9), dict(epsilon=np.inf),
               dict(epsilon=np.nan), dict(enable=2), dict(frozen=2), dict(frozen=-1)):
        _expect(wk, -1, lambda kw=kw: on.reward_norm(**kw))
    for a in ((-1, 0.0, 0.0), (1, np.nan, 0.0), (1, np.inf, 0.0), (1, 0.0, -1.0), (1, 0.0, np.nan), (1, 0.0, np.inf)):
        _expect(wk, -1, on.set_reward_norm_state, *a)
    assert on.reward_norm_state() == before
    # a disable keeps the state for a later enable
    on.reward_norm(enable=False)
    assert on.reward_norm_state()["enabled"] == 0
    on.reward_norm()
    s = on.reward_norm_state()
    assert _rec_bytes(s) == _rec_bytes(before) and s["enabled"] == 1
    for e in (on, off, comm):
        e.close()
