"""GPU, one process: the record exchange (wk_comm_records) with one rank, where the fold is the
identity -- a TargetKL + LearnLogStd + reward-normalisation context behind the host callback or
RCCL must reach the bytes of the same context without a communicator -- and the raw sums
(wk_policy_sums), the refusals and the failures of the exchange.

272 walkers x horizon 11: two reward-normalisation tiles (256 + 16, the second partial), the scan's
unrolled body and its tail (8 + 3), and 2,992 rows = 187 sixteen-row chunks of the statistics kernel.
"""
import numpy as np
import pytest

import sumsref
from conftest import SEED

pytestmark = pytest.mark.gpu

N, T, MB = 272, 11, 748  # four minibatches per epoch
CFG = dict(Horizon=T, Minibatch=MB, Epochs=3, RandomizeStart=1, RandomizeMaterial=1)
FULL = dict(CFG, TargetKL=1e30, LearnLogStd=1, EntropyCoef=0.01)


def _expect(wk, code, fn, *a, word=None):
    with pytest.raises(wk.WkError) as ex:
        fn(*a)
    assert f"({code})" in str(ex.value), str(ex.value)
    if word:
        assert word in str(ex.value), str(ex.value)


def _bytes(d):
    return {k: np.array([v]).tobytes() for k, v in d.items()}


def _state(e):
    """everything the ranks must agree on, as bytes"""
    m, v, t = e.get_adam()
    return dict(w=e.get_weights().tobytes(), m=m.tobytes(), v=v.tobytes(), t=t, log_std=_bytes(e.log_std()),
                rnorm=_bytes(e.reward_norm_state()), scaled=e.scaled_rewards().tobytes(),
                upd=_bytes(e.update_stats()))


def _train(e, iterations=2):
    out = []
    for u in range(iterations):
        e.rollout(T)
        e.ppo_update(update_index=u)
        out.append(_state(e))
    return out


@pytest.fixture(scope="module")
def solo_states(wk):
    """context A: every control on, no communicator -- computed once, shared, left unchanged"""
    a = wk.Engine(N, seed=SEED, **FULL)
    a.reward_norm()
    st = _train(a)
    a.close()
    return st


def _identity(i):
    """a one-rank all-gather: the rank's own record is every rank's"""
    return i.reshape(1, -1)


def test_one_rank_host_exchange_is_the_identity(wk, solo_states):
    seen = []

    def gather(mine):
        seen.append(mine.copy())
        return _identity(mine)

    b = wk.Engine(N, seed=SEED, **FULL)
    b.reward_norm()  # (enabled before the communicator: the initialiser must accept it)
    b.comm_records(gather)
    b.comm_init_host(0, 1, lambda buf: None)
    assert b.comm_info()[0] == "host"
    got = _train(b)
    for it, (x, y) in enumerate(zip(got, solo_states)):
        for k in y:
            assert x[k] == y[k], (it, k)
    assert got[1]["upd"] != got[0]["upd"] and got[1]["rnorm"] != got[0]["rnorm"]
    # one exchange per rollout (kind 2) and one per epoch (kind 1), numbered consecutively
    assert len(seen) == 2 * (1 + 3)
    hdr = [int(r[0]) for r in seen]
    assert [h >> 56 for h in hdr] == [2, 1, 1, 1] * 2
    assert [(h >> 48) & 0xFF for h in hdr] == [1] * 8
    assert [h & ((1 << 48) - 1) for h in hdr] == list(range(8))
    assert all(r.shape == (wk.COMM_RECORD_WORDS,) and r.dtype == np.uint64 for r in seen)
    # a reward-normalisation record: count + bad = the pass's samples, the rest of the record zero
    assert int(seen[0][1]) + int(seen[0][2]) == N * T and not seen[0][5:].any()
    assert not seen[1][14:].any() and int(seen[1][1]) + int(seen[1][2]) == N * T  # rows + skipped
    # enabling after the communicator exists is allowed on such a context, and still collective
    c = wk.Engine(N, seed=SEED, **FULL)
    c.comm_records(gather)
    c.comm_init_host(0, 1, lambda buf: None)
    c.reward_norm()
    c.rollout(T)
    assert c.scaled_rewards().tobytes() == solo_states[0]["scaled"]
    assert c.reward_norm_state()["scale"] != 1.0 and [int(r[0]) >> 56 for r in seen[8:]] == [2]
    for e in (b, c):
        e.close()


def test_one_rank_rccl_exchange_is_the_identity(wk, solo_states):
    b = wk.Engine(N, seed=SEED, **FULL)
    b.comm_records(None)
    b.comm_init(0, 1, wk.Engine.comm_unique_id())
    assert b.comm_info()[0] == "rccl"
    b.reward_norm()
    got = _train(b)
    for it, (x, y) in enumerate(zip(got, solo_states)):
        for k in y:
            assert x[k] == y[k], (it, k)
    b.sync()  # (reports a pending header check: none)
    b.close()


def test_policy_sums(wk):
    e = wk.Engine(N, seed=SEED, **dict(FULL, TargetKL=0.0))
    e.rollout(T)
    e.ppo_update(update_index=0)  # (moves the policy off the one that collected the data)
    s = e.policy_sums()
    assert s["rows"] + s["skipped"] == N * T and s["kl"] > 0 and s["zz"] > 0
    assert sumsref.same_bytes(wk.stats_from_sums(s), e.policy_stats(), sumsref.STATS_KEYS)
    assert sumsref.same_bytes(wk.log_std_grad_from_sums(s, 0.01), e.log_std_gradient(), sumsref.GRAD_KEYS)
    assert sumsref.same_bytes(sumsref.stats_from_sums(s), e.policy_stats(), sumsref.STATS_KEYS)
    loc, glo = e.policy_sums(global_=True)
    assert sumsref.same_bytes(loc, s, sumsref.FIELDS) and sumsref.same_bytes(glo, s, sumsref.FIELDS)
    assert sumsref.same_bytes(e.policy_stats_global(), e.policy_stats(), sumsref.STATS_KEYS)
    # a communicator without the opt-in: the local record as before, no global one
    h = wk.Engine(N, seed=SEED, **CFG)
    h.comm_init_host(0, 1, lambda buf: None)
    _expect(wk, -5, h.policy_sums)  # (no trajectory yet)
    h.rollout(T)
    assert h.policy_sums()["rows"] + h.policy_sums()["skipped"] == N * T
    _expect(wk, -5, h.policy_sums, True, word="wk_comm_records")
    _expect(wk, -5, h.policy_stats_global)
    # with it, one rank: the global record is the local one, through one exchange
    calls = []
    r = wk.Engine(N, seed=SEED, **CFG)
    r.comm_records(lambda mine: (calls.append(int(mine[0])), _identity(mine))[1])
    r.comm_init_host(0, 1, lambda buf: None)
    r.rollout(T)
    loc, glo = r.policy_sums(global_=True)
    assert sumsref.same_bytes(loc, glo, sumsref.FIELDS) and calls == [1 << 56 | 1 << 48]
    assert sumsref.same_bytes(loc, h.policy_sums(), sumsref.FIELDS)  # (same seed, same shard)
    for x in (e, h, r):
        x.close()


def test_refusals(wk):
    gather = _identity
    e = wk.Engine(N, seed=SEED, **FULL)
    # after an initialiser
    late = wk.Engine(N, seed=SEED, **CFG)
    late.comm_init_host(0, 1, lambda buf: None)
    _expect(wk, -5, late.comm_records, gather)
    _expect(wk, -5, late.comm_records, None)
    # the initialiser must match the declared kind; twice is an error
    host = wk.Engine(N, seed=SEED, **FULL)
    host.comm_records(gather)
    _expect(wk, -5, host.comm_records, gather)
    _expect(wk, -5, host.comm_init, 0, 1, bytes(128))
    host.comm_init_host(0, 1, lambda buf: None)
    rccl = wk.Engine(N, seed=SEED, **FULL)
    rccl.comm_records(None)
    _expect(wk, -5, rccl.comm_init_host, 0, 1, lambda buf: None)
    assert rccl.comm_info()[0] == "none"
    # the general networks stay one GPU
    gen = wk.Engine(N, seed=SEED, **dict(CFG, NetworkKernels=1))
    _expect(wk, -3, gen.comm_records, None)
    _expect(wk, -3, gen.comm_records, gather)
    # the IPC exchange stays closed, with and without the opt-in
    _expect(wk, -3, e.comm_ipc_handle)
    e.comm_records(gather)
    _expect(wk, -3, e.comm_ipc_handle)
    _expect(wk, -3, e.comm_init_ipc_records, 0, 1, [bytes(wk.IPC_HANDLE_BYTES)])
    rn = wk.Engine(N, seed=SEED, **CFG)
    rn.reward_norm()
    rn.comm_records(None)
    _expect(wk, -3, rn.comm_ipc_handle)
    # without the opt-in: as before
    plain = wk.Engine(N, seed=SEED, **FULL)
    _expect(wk, -3, plain.comm_init_host, 0, 1, lambda buf: None)
    for x in (e, late, host, rccl, gen, rn, plain):
        x.close()


def test_failing_gather_takes_no_step(wk):
    """the callback fails in epoch 2's exchange: WK_ERR_COMM, and the log-std and its Adam state are
    those after epoch 1"""
    calls = []

    def gather(mine):
        calls.append(int(mine[0]) >> 56)
        if calls.count(1) == 2:
            raise ConnectionError("peer 1 went away")
        return _identity(mine)

    def make(g):
        e = wk.Engine(N, seed=SEED, **FULL)
        e.comm_records(g)
        e.comm_init_host(0, 1, lambda buf: None)
        e.reward_norm()
        e.rollout(T)
        return e

    ref = make(_identity)
    ref.ppo_update(epochs=1, update_index=0)
    e = make(gather)
    with pytest.raises(wk.WkError, match="ConnectionError: peer 1 went away") as ex:
        e.ppo_update(update_index=0)
    assert "(-4)" in str(ex.value) and calls == [2, 1, 1]
    a, b = e.log_std(), ref.log_std()
    assert b["t"] == 1 and b["steps"] == 1
    assert _bytes(a) == _bytes(b)
    for x in (e, ref):
        x.close()


def test_wrong_sequence_number_names_the_rank(wk):
    def gather(mine):
        out = _identity(mine).copy()
        if int(mine[0]) >> 56 == 1:
            out[0, 0] += np.uint64(1)  # rank 0's slot carries the next exchange's number
        return out

    e = wk.Engine(N, seed=SEED, **FULL)
    e.comm_records(gather)
    e.comm_init_host(0, 1, lambda buf: None)
    e.rollout(T)
    before = _bytes(e.log_std())
    with pytest.raises(wk.WkError, match="rank 0's record") as ex:
        e.ppo_update(update_index=0)
    assert "(-4)" in str(ex.value)
    assert _bytes(e.log_std()) == before  # no step was taken
    # the same in the reward normalisation's exchange: the rollout fails, nothing is merged
    f = wk.Engine(N, seed=SEED, **CFG)
    f.comm_records(lambda mine: _identity(mine) + np.uint64(1 << 48))  # another number of ranks
    f.comm_init_host(0, 1, lambda buf: None)
    f.reward_norm()
    _expect(wk, -4, f.rollout, T, word="rank 0's record")
    assert f.reward_norm_state()["count"] == 0
    for x in (e, f):
        x.close()
