"""The flat-floor pair kernels take the polygons' vertices one at a time (WK_VERTEX_PACKED 0 in
csrc/wk_env_pair.hip, read by csrc/wk_device.h: move, rotate, proj_minmax, pole_own_minmax),
every other kernel two at a time through v_pk_add_f32 / v_pk_mul_f32.  The two forms are the same
IEEE operations per element, so the side kernels must still equal the one-lane kernel
k_env_step<..., 1> (packed) bit for bit:

- 33 walkers (a partial wave of the pair mapping) and 160 (more than one block), LanesPerWalker 2
  (pair, per vertex) and 4 (quad, packed), RandomizeStart, uniform seeded actions, 12 env-steps with
  MaxTimesteps 8: observations, rewards, dones, fault flags and the final walker records.
- The CPU oracle confirms (no GPU needed) that these runs hold leg-leg and leg-floor contacts, a
  reset of every walker and floor candidates after the reset, so move / rotate / both projections
  run on every path and a segment's pairs are visited in both list orders.
"""
import numpy as np
import pytest

SEED = 20250905
T, MAX_TIMESTEPS, ACTION_SEED = 12, 8, 7
SHAPES = (33, 160)
LEG_LEG, LEG_FLOOR = [0, 2, 5, 7], [1, 3, 6, 8]  # the candidate pairs' trace slots


def _actions(n):
    return np.random.default_rng(ACTION_SEED).uniform(-1.0, 1.0, (T, n, 4)).astype(np.float32)


@pytest.mark.parametrize("n", SHAPES)
def test_runs_hold_contacts_and_a_reset(orc, n):
    """the oracle's trace of the same runs: leg-leg and leg-floor contacts, every walker reset
    once (MaxTimesteps 8 < 12 steps), and a floor candidate past the box test after the reset"""
    dx, _ = orc.env_setup(SEED, n)
    acts = _actions(n)
    leg_leg = leg_floor = resets = post_floor = 0
    for i in range(n):
        e = orc.Env(dx=dx[i], material=0, MaxTimesteps=MAX_TIMESTEPS)
        was_reset = False
        for t in range(T):
            _, _, done, tr = e.step(acts[t, i], trace=True)
            leg_leg += int((tr["n_contacts"][:, LEG_LEG] > 0).any())
            leg_floor += int((tr["n_contacts"][:, LEG_FLOOR] > 0).any())
            post_floor += int(was_reset and tr["aabb_hit"][:, LEG_FLOOR].any())
            resets += int(done)
            was_reset |= bool(done)
    assert leg_leg > n and leg_floor > n and resets == n and post_floor > 0, (leg_leg, leg_floor, resets, post_floor)


def _run(wk, n, lanes):
    eng = wk.Engine(n, seed=SEED, Horizon=T, Minibatch=n * T // 4, Epochs=1, RandomizeStart=1,
                    MaxTimesteps=MAX_TIMESTEPS, LanesPerWalker=lanes)
    obs, rew, done, fault = eng.step(_actions(n), k=T)
    state = eng.get_state()
    eng.close()
    return obs, rew, done, fault, state


_REFERENCE = {}


def _reference(wk, n):
    if n not in _REFERENCE:
        _REFERENCE[n] = _run(wk, n, 1)
    return _REFERENCE[n]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("n", SHAPES)
def test_side_kernels_equal_the_one_lane_kernel(wk, n, lanes):
    ref = _reference(wk, n)
    assert ref[2].sum() == n and not ref[3].any()  # every walker reset once, no fault
    got = _run(wk, n, lanes)
    for name, a, b in zip(("observations", "rewards", "dones", "fault", "walker records"), got, ref):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=name)
