"""GPU: wk_evaluate -- deterministic (or sampled) complete-episode evaluation on a private copy of
the walkers -- on both kernel families.  tests/evalref.py holds the end-kind rule, the float64
aggregation and the shared case (tests/test_evalref.py checks them on the oracle).

  1. emulation, bit for bit: evaluate(records=True) against a second context of the same seed and
     weights driven through the public calls (reset, then get_obs -> policy_sample -> step per
     env-step; rewards summed in double on the host).  The oracle replays that context's actions
     (the physics is bit-exact: its rewards and dones are asserted equal) and supplies the torso x
     the public step does not return, so every field of every record is compared in every bit;
  2. against wk_rollout's episode log on a general context (the kernels are the same);
  3. no side effects on a training sequence;
  4. the fold at its edges (wave, block tile, grid pass) against evalref, and repeatability;
  5. stopping and argument errors.
Every case prints its figures (pytest -s)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import evalref
import netref

pytestmark = pytest.mark.gpu

SEED = 20250905
F = np.float32
PROP = dict(shape="Square", smooth=1, material="Wood", is_static=False, cx=150, cy=700, size=30, ay=980)
# (name, config, stochastic, rng_step0): the shared case and its variants
VARIANTS = {
    "base": (dict(MaxTimesteps=evalref.CASE_MT), False, 0),
    "sampled": (dict(MaxTimesteps=40), True, 7),
    "rough": (dict(MaxTimesteps=evalref.CASE_MT, RoughFloor=1), False, 0),
    "prop": (dict(MaxTimesteps=evalref.CASE_MT), False, 0),
    "odd": (dict(MaxTimesteps=evalref.CASE_MT, NetworkKernels=1, CriticNeuralNetwork=netref.NETS["odd"][0],
                 ActorNeuralNetwork=netref.NETS["odd"][1]), False, 0),
}


def _case_engine(wk, orc, variant, **extra):
    cfg, _, _ = VARIANTS[variant]
    eng = wk.Engine(evalref.CASE_N, seed=SEED, Horizon=4, **cfg, **extra)
    eng.set_offsets(evalref.case_offsets(orc, SEED))
    if variant == "prop":
        eng.set_scene([wk.make_prop(**PROP)])
    eng.set_weights(evalref.case_weights(nparam=eng.nparam))
    return eng


@functools.lru_cache(maxsize=None)
def _emulated(wk, orc, variant, episodes=evalref.CASE_EPISODES):
    """(records [episodes][n], env-steps needed) of the second context driven through the public
    calls, the torso x from the oracle's replay of its actions.  Computed once per variant."""
    cfg, stochastic, step0 = VARIANTS[variant]
    mt, n = cfg["MaxTimesteps"], evalref.CASE_N
    eng = _case_engine(wk, orc, variant)
    dx = evalref.case_offsets(orc, SEED)
    props = [orc.make_prop(**PROP)] if variant == "prop" else ()
    envs = [orc.Env(dx=float(dx[i]), rough=(SEED, i) if cfg.get("RoughFloor") else None, props=props,
                    MaxTimesteps=mt) for i in range(n)]
    for e in envs:
        e.reset()
    eng.reset()
    runs = [evalref.Running(i, episodes, mt) for i in range(n)]
    t = 0
    while not all(r.done() for r in runs):
        assert t < episodes * (mt + 1), "a walker did not finish within episodes * (MaxTimesteps + 1)"
        obs = eng.get_obs()
        mean, act, _ = eng.policy_sample(obs, steps=np.full(n, step0 + t, np.uint32))
        a = act if stochastic else mean
        _, rew, done, _ = eng.step(a[None], 1)
        for i, e in enumerate(envs):
            assert np.array_equal(obs[i], e.obs()), (variant, t, i)
            _, r, d = e.step(a[i])
            assert F(r).tobytes() == rew[0, i].tobytes() and d == done[0, i], (variant, t, i)
            runs[i].add(rew[0, i], done[0, i], e.step_position()[0])
        t += 1
    eng.close()
    return evalref.records_array(runs, episodes), t


def _assert_records_equal(got, ref, tag):
    for k in ref.dtype.names:
        assert got[k].tobytes() == ref[k].tobytes(), (tag, k, got[k], ref[k])


def _stats_bytes(st):
    return [(k, np.float64(v).tobytes() if isinstance(v, float) else int(v)) for k, v in st.items()]


def _check_stats(st, recs, n, tag):
    """the folded statistics against evalref's aggregation of the same records: counts and extrema
    exact, the integer length mean exact, the double sums within 4 N 2^-53 sum|x| of math.fsum"""
    ref = evalref.aggregate(recs)
    for k in ("episodes", "unfinished", "fell", "timed_out", "succeeded", "length_min", "length_max"):
        assert st[k] == ref[k], (tag, k, st[k], ref[k])
    c = ref["episodes"]
    floats = ("reward_mean", "reward_std", "reward_min", "reward_max", "length_mean", "distance_mean", "distance_max")
    if c == 0:
        assert all(math.isnan(st[k]) for k in floats), (tag, st)
        return ref
    fin = recs.reshape(-1)[recs.reshape(-1)["end"] != evalref.UNFINISHED]
    x = [float(v) for v in fin["total_reward"]]
    d = [float(v) for v in fin["distance"]]
    for k in ("reward_min", "reward_max", "distance_max", "length_mean"):
        assert st[k] == ref[k], (tag, k, st[k], ref[k])
    bx, bd, bxx = evalref.sum_bound(x) / c, evalref.sum_bound(d) / c, evalref.sum_bound([v * v for v in x]) / c
    m, s2 = ref["reward_mean"], math.fsum(v * v for v in x) / c
    # variance = S2 / c - mean^2 from sums within their bounds, the two terms and the square of the
    # returned std each rounded to 2^-53 of their size
    bvar = bxx + 2 * abs(m) * bx + bx * bx + 4 * 2.0 ** -53 * (s2 + m * m)
    var_ref = max(0.0, s2 - m * m)
    fig = dict(reward_mean=(st["reward_mean"] - m, bx), distance_mean=(st["distance_mean"] - ref["distance_mean"], bd),
               reward_var=(st["reward_std"] ** 2 - var_ref, bvar + 4 * 2.0 ** -53 * var_ref))
    print(tag, "fold:", {k: f"{abs(a):.3g} / {b:.3g}" for k, (a, b) in fig.items()})
    for k, (a, b) in fig.items():
        assert abs(a) <= b, (tag, k, a, b)
    return ref


# ---------------------------------------------------------------- 1. emulation, bit for bit
@pytest.mark.parametrize("variant,lanes", [("base", 1), ("base", 2), ("base", 4), ("sampled", 0),
                                           ("rough", 0), ("prop", 0), ("odd", 0)])
def test_evaluate_equals_the_public_calls(wk, orc, variant, lanes):
    _, stochastic, step0 = VARIANTS[variant]
    ref, needed = _emulated(wk, orc, variant)
    kinds = np.bincount(ref["end"].reshape(-1), minlength=4).tolist()
    print(variant, "lanes", lanes, "emulated kinds [fell, limit, success, unfinished]:", kinds, "steps needed:", needed)
    if variant == "base":  # (evalref.CASE_WEIGHT_SEED: the GPU policy's rounding may move falls)
        assert kinds[evalref.FELL] > 0 and kinds[evalref.TIME_LIMIT] > 0 and kinds[evalref.SUCCESS] > 0, kinds
    assert kinds[evalref.UNFINISHED] == 0
    eng = _case_engine(wk, orc, variant, LanesPerWalker=lanes)
    st, recs = eng.evaluate(episodes=evalref.CASE_EPISODES, stochastic=stochastic, rng_step0=step0, poll=1,
                            records=True)
    _assert_records_equal(recs, ref, (variant, lanes))
    assert st["steps_run"] == needed and st["env_steps"] == needed * evalref.CASE_N and st["fault_or"] == 0
    _check_stats(st, recs, evalref.CASE_N, (variant, lanes))
    eng.close()


# ---------------------------------------------------------------- 2. against the rollout
def test_evaluate_equals_the_rollout_on_a_general_context(wk):
    n, T, K = 17, 24, 4
    cfg = dict(NetworkKernels=1, CriticNeuralNetwork=netref.NETS["odd"][0], ActorNeuralNetwork=netref.NETS["odd"][1],
               MaxTimesteps=5, Horizon=T, RandomizeStart=1)
    a, b = wk.Engine(n, seed=SEED, **cfg), wk.Engine(n, seed=SEED, **cfg)
    w = np.random.default_rng(11).normal(0, 0.3, a.nparam).astype(F)
    a.set_weights(w)
    b.set_weights(w)
    a.rollout(T)
    log, dropped = a.drain_episodes()
    assert dropped == 0 and len(log) == K * n, len(log)
    st, recs = b.evaluate(episodes=K, stochastic=True, start="create", rng_step0=0, records=True)
    assert st["episodes"] == K * n and st["steps_run"] == T
    for e in range(n):
        mine = log[log["env"] == e]  # completion order
        assert len(mine) == K
        assert mine["total_reward"].tobytes() == recs["total_reward"][:, e].tobytes(), e
        assert mine["length"].tobytes() == recs["length"][:, e].tobytes(), e
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. no side effects
def _observable(eng, T, returns_mode):
    tr = eng.get_trajectory(T)
    m, v, t = eng.get_adam()
    rs = eng.rollout_stats()
    out = dict(state=eng.get_state(), weights=eng.get_weights(), adam_m=m, adam_v=v, adam_t=np.int64(t),
               rollout_stats=np.frombuffer(bytes(rs), np.uint8), **{"traj_" + k: x for k, x in tr.items()})
    if returns_mode:
        out["bootstrap"] = eng.get_bootstrap_values()
    return out


@pytest.mark.parametrize("family,returns_mode", [("builtin", 0), ("builtin", 1), ("general", 0)])
def test_evaluate_leaves_the_training_run_alone(wk, family, returns_mode):
    """two contexts of one seed run rollout, rollout, ppo_update and drain their logs; one also
    evaluates (deterministic and sampled) after the first rollout and before the update.
    Everything a later call can observe is equal in every byte.  The profile: its launch and
    env-step counts are equal across the contexts, and on the evaluating context the whole
    record, the millisecond totals included, has the same bytes before and after each evaluate
    (two contexts' millisecond totals are two measurements and cannot be compared)"""
    n, T = 33, 8
    cfg = dict(Horizon=T, MaxTimesteps=5, RandomizeStart=1, ReturnsMode=returns_mode)
    if family == "general":
        cfg.update(NetworkKernels=1, CriticNeuralNetwork=netref.NETS["odd"][0], ActorNeuralNetwork=netref.NETS["odd"][1])
    engs = [wk.Engine(n, seed=SEED, **cfg) for _ in range(2)]
    w = np.random.default_rng(5).normal(0, 0.3, engs[0].nparam).astype(F)
    seen, snap = [], []

    def evaluate(eng):
        before = bytes(_profile_struct(wk, eng))
        eng.evaluate(episodes=2)
        eng.evaluate(episodes=1, stochastic=True, rng_step0=3, start="create", records=True)
        assert bytes(_profile_struct(wk, eng)) == before

    for i, eng in enumerate(engs):
        eng.set_weights(w)
        eng.profile_enable(1)
        eng.rollout(T)
        eng.snapshot()
        snap.append((eng.get_state(), eng.get_weights()))
        if i == 1:
            evaluate(eng)
        eng.rollout(T)
        if i == 1:
            evaluate(eng)
        eng.ppo_update(update_index=0)
        obs = _observable(eng, T, returns_mode)
        ep, dropped = eng.drain_episodes()
        cl, al = eng.drain_losses()
        obs.update(episodes=ep, dropped=np.int64(dropped), critic_losses=cl, actor_losses=al)
        prof = eng.profile()
        obs["profile_counts"] = np.array([v for k, v in prof.items() if not k.endswith("_ms")], np.int64)
        assert prof["physics_launches"] == 2 and prof["physics_env_steps"] == 2 * n * T
        seen.append(obs)
    assert len(seen[0]["episodes"]) > 0 and len(seen[0]["critic_losses"]) == 1
    for k in seen[0]:
        assert np.asarray(seen[0][k]).tobytes() == np.asarray(seen[1][k]).tobytes(), k
    # the snapshot taken before the evaluations still restores
    for eng, (st0, w0) in zip(engs, snap):
        eng.restore()
        assert eng.get_state().tobytes() == st0.tobytes() and eng.get_weights().tobytes() == w0.tobytes()
        eng.close()


def _profile_struct(wk, eng):
    p = wk.Profile()
    eng._chk(eng.lib.wk_profile_get(eng.h, C.byref(p)), "wk_profile_get")
    return p


# ---------------------------------------------------------------- 4. fold edges, repeatability
# one lane per walker: 63 / 64 / 65 straddle a wave, 257 is one walker past the fold's block tile
# (EVAL_FOLD_BLOCK = 256), 16,385 one past a whole pass of its capped grid (64 blocks of 256)
FOLD_N = (1, 63, 64, 65, 257, 16385)


@pytest.mark.parametrize("n", FOLD_N)
def test_fold_edges_and_repeatability(wk, n):
    assert wk.EVAL_FOLD_BLOCK + 1 in FOLD_N and wk.EVAL_FOLD_BLOCK * wk.EVAL_FOLD_MAX_BLOCKS + 1 in FOLD_N
    cfg = dict(MaxTimesteps=5, Horizon=2, RandomizeStart=1, EnvOffset=5)
    eng = wk.Engine(n, seed=SEED, **cfg)
    w = np.random.default_rng(7).normal(0, 0.3, eng.nparam).astype(F)
    eng.set_weights(w)
    st, recs = eng.evaluate(episodes=3, stochastic=True, records=True)
    assert recs.shape == (3, n) and (recs["env"] == 5 + np.arange(n)[None]).all()
    assert st["episodes"] == 3 * n and st["unfinished"] == 0 and st["fault_or"] == 0
    assert st["env_steps"] == st["steps_run"] * n and st["length_max"] <= 6
    for r in recs.reshape(-1):
        assert r["end"] == evalref.end_kind(r["final_x"], r["length"], 5)
    assert len(np.unique(recs["total_reward"])) > 1 or n == 1
    _check_stats(st, recs, n, ("fold", n))
    st2, recs2 = eng.evaluate(episodes=3, stochastic=True, records=True)
    assert _stats_bytes(st2) == _stats_bytes(st) and recs2.tobytes() == recs.tobytes()
    # a smaller call after the larger one sees nothing of it: it equals a fresh context's
    small = eng.evaluate(episodes=1, stochastic=True, rng_step0=2, records=True)
    eng.close()
    fresh = wk.Engine(n, seed=SEED, **cfg)
    fresh.set_weights(w)
    want = fresh.evaluate(episodes=1, stochastic=True, rng_step0=2, records=True)
    fresh.close()
    assert _stats_bytes(small[0]) == _stats_bytes(want[0]) and small[1].tobytes() == want[1].tobytes()
    assert small[1].tobytes() != recs[:1].tobytes()  # (another Philox step: other episodes)


# ---------------------------------------------------------------- 5. stopping and errors
def test_stopping(wk, orc):
    ref, needed = _emulated(wk, orc, "base")
    n, K = evalref.CASE_N, evalref.CASE_EPISODES
    eng = _case_engine(wk, orc, "base")
    runs = {}
    for poll, cap in ((1, 1000), (32, 1000), (1000, 1000), (100, needed + 8), (0, 0)):
        st, recs = eng.evaluate(episodes=K, poll=poll, max_steps=cap, records=True)
        p, m = poll or 32, cap or K * (evalref.CASE_MT + 1)
        want = min(-(-needed // p) * p, m)
        print("poll", poll, "max_steps", cap, "steps_run", st["steps_run"], "needed", needed)
        assert st["steps_run"] == want and st["env_steps"] == want * n, (poll, cap, st["steps_run"], want)
        runs[(poll, cap)] = recs
    for k, recs in runs.items():  # the steps after a walker's last episode are ignored
        assert recs.tobytes() == runs[(1, 1000)].tobytes(), k
    _assert_records_equal(runs[(1, 1000)], ref, "poll")
    # episodes = 2 from the reset state, deterministic: round 1 repeats round 0
    assert runs[(1, 1000)][1].tobytes() == runs[(1, 1000)][0].tobytes()
    # a cap no walker finishes within (walker 3's success aside: moved back for this call)
    dx = evalref.case_offsets(orc, SEED)
    dx[evalref.CASE_GOAL_WALKER] = 0.0
    eng.set_offsets(dx)
    st, recs = eng.evaluate(episodes=K, max_steps=10, records=True)
    assert st["steps_run"] == 10 and st["episodes"] == 0 and st["unfinished"] == K * n
    assert (recs["end"] == evalref.UNFINISHED).all()
    z = recs.copy()
    z["end"] = 0
    assert not z.tobytes().strip(b"\0")  # zero otherwise
    for k in ("reward_mean", "reward_std", "reward_min", "reward_max", "length_mean", "distance_mean", "distance_max"):
        assert math.isnan(st[k]), (k, st[k])
    assert st["length_min"] == 0 and st["length_max"] == 0 and st["fell"] == st["timed_out"] == st["succeeded"] == 0
    eng.close()


def test_max_steps_10_on_the_shared_case(wk, orc):
    """the issue's case as it stands (walker 3 next to the goal succeeds on its first step, and
    again after each reset): every other slot is UNFINISHED"""
    eng = _case_engine(wk, orc, "base")
    st, recs = eng.evaluate(episodes=evalref.CASE_EPISODES, max_steps=10, records=True)
    g = evalref.CASE_GOAL_WALKER
    others = np.delete(recs, g, axis=1)
    assert (others["end"] == evalref.UNFINISHED).all() and (recs[:, g]["end"] == evalref.SUCCESS).all()
    assert st["episodes"] == evalref.CASE_EPISODES and st["unfinished"] == others.size and st["steps_run"] == 10
    _check_stats(st, recs, evalref.CASE_N, "max_steps=10")
    eng.close()


def test_argument_errors(wk):
    eng = wk.Engine(8, seed=SEED, Horizon=2, MaxTimesteps=5)
    for bad in (dict(episodes=wk.EVAL_MAX_EPISODES + 1), dict(episodes=-1), dict(max_steps=-1), dict(poll=-1)):
        with pytest.raises(wk.WkError, match=r"wk_evaluate failed \(-1\)"):
            eng.evaluate(**bad)
    args, st = wk.EvalArgs(), wk.EvalStats()
    assert eng.lib.wk_evaluate(eng.h, C.byref(args), None, None) == -1          # NULL out
    assert eng.lib.wk_evaluate(None, C.byref(args), C.byref(st), None) == -1     # NULL context
    assert eng.lib.wk_evaluate(eng.h, None, C.byref(st), None) == 0              # NULL args: the defaults
    assert st.episodes == 8 and st.steps_run == 6                                # one episode each, 1 * (5 + 1) steps
    st16 = eng.evaluate(episodes=wk.EVAL_MAX_EPISODES)
    assert st16["episodes"] == 8 * wk.EVAL_MAX_EPISODES
    with pytest.raises(wk.WkError, match=r"\(-5\)"):
        wk.Engine(8, seed=SEED, Horizon=2).evaluate_time(4)                      # before any evaluate
    step_ms, fold_ms = eng.evaluate_time(4)
    assert step_ms > 0 and fold_ms > 0
    eng.close()
