"""CPU: the evaluation reference (tests/evalref.py) -- the end-kind rule and the float64
aggregation -- on oracle-driven complete episodes.  The case is the one tests/test_gpu_eval.py
emulates on the GPU: 24 walkers at the seed's RandomizeStart offsets, walker 3 next to the goal,
MaxTimesteps 120, weights default_rng(4).normal(0, 0.5), Env.reset() first, Agent.mean, two
episodes each.  The oracle gives per round 13 falls (lengths 58..113), 10 time limits (121) and
one success (length 1, reward about 80); the counts are not pinned here."""
import math

import numpy as np
import pytest

import evalref
from conftest import SEED


@pytest.fixture(scope="module")
def case(orc):
    dx = evalref.case_offsets(orc, SEED)
    recs, needed = evalref.oracle_episodes(orc, dx, evalref.case_weights(), evalref.CASE_EPISODES,
                                           evalref.CASE_MT)
    return recs, needed


def test_end_kind_rule():
    mt = 120
    assert evalref.end_kind(900.5, 1, mt) == evalref.SUCCESS
    assert evalref.end_kind(np.float32(900.0), 50, mt) == evalref.FELL          # strictly past the line
    assert evalref.end_kind(np.nextafter(np.float32(900.0), np.float32(1e9)), 50, mt) == evalref.SUCCESS
    assert evalref.end_kind(901.0, mt + 1, mt) == evalref.SUCCESS                # the goal wins over the limit
    assert evalref.end_kind(300.0, mt + 1, mt) == evalref.TIME_LIMIT
    assert evalref.end_kind(300.0, mt, mt) == evalref.FELL
    assert evalref.end_kind(float("nan"), 7, mt) == evalref.FELL                 # NaN > 900 is false


def test_oracle_case_has_every_kind_and_repeats(case):
    recs, needed = case
    assert recs.shape == (evalref.CASE_EPISODES, evalref.CASE_N)
    ends = recs["end"]
    print("ends per round:", [np.bincount(ends[k], minlength=4).tolist() for k in range(2)],
          "lengths of falls:", sorted(recs["length"][0][ends[0] == evalref.FELL].tolist()), "steps needed:", needed)
    assert (ends != evalref.UNFINISHED).all()
    for kind in (evalref.FELL, evalref.TIME_LIMIT, evalref.SUCCESS):
        assert (ends[0] == kind).any(), kind
    # every reset returns a deterministic walker to the same state: round 1 repeats round 0
    assert recs[1].tobytes() == recs[0].tobytes()
    # what the kinds mean
    assert (recs["length"][ends == evalref.TIME_LIMIT] == evalref.CASE_MT + 1).all()
    assert (recs["length"][ends == evalref.FELL] <= evalref.CASE_MT).all()
    assert (recs["final_x"][ends == evalref.SUCCESS] > 900.0).all()
    goal = recs[0, evalref.CASE_GOAL_WALKER]
    assert goal["end"] == evalref.SUCCESS and goal["length"] == 1 and 79.0 < goal["total_reward"] < 82.0
    assert (recs["distance"] >= recs["final_x"]).all() and (recs["env"][0] == np.arange(evalref.CASE_N)).all()
    assert needed == recs["length"].sum(axis=0).max()


def test_aggregation_against_fsum(case):
    recs, _ = case
    # an unfinished slot is counted and left out of every statistic
    r = recs.copy()
    r[1, 5] = np.zeros((), evalref.REC_DTYPE)
    r[1, 5]["end"] = evalref.UNFINISHED
    got = evalref.aggregate(r)
    fin = [x for x in r.reshape(-1) if x["end"] != evalref.UNFINISHED]
    c = len(fin)
    assert got["episodes"] == c == r.size - 1 and got["unfinished"] == 1
    assert got["fell"] + got["timed_out"] + got["succeeded"] == c
    x = [float(v["total_reward"]) for v in fin]
    assert got["reward_mean"] == math.fsum(x) / c
    var = math.fsum(v * v for v in x) / c - (math.fsum(x) / c) ** 2
    assert got["reward_std"] == math.sqrt(max(0.0, var))
    assert got["reward_min"] == min(x) and got["reward_max"] == max(x)
    assert got["length_mean"] == sum(int(v["length"]) for v in fin) / c
    assert got["length_min"] == min(int(v["length"]) for v in fin)
    assert got["length_max"] == max(int(v["length"]) for v in fin) == evalref.CASE_MT + 1
    assert got["distance_mean"] == math.fsum(float(v["distance"]) for v in fin) / c
    assert got["distance_max"] == max(float(v["distance"]) for v in fin) > 900.0
    # numpy's pairwise float64 mean agrees within the ordered-sum bound
    assert abs(np.mean(np.array(x)) - got["reward_mean"]) <= evalref.sum_bound(x) / c
    # no finished episode: counts 0, every mean NaN
    r["end"] = evalref.UNFINISHED
    none = evalref.aggregate(r)
    assert none["episodes"] == 0 and none["unfinished"] == r.size
    assert all(math.isnan(none[k]) for k in ("reward_mean", "reward_std", "reward_min", "reward_max",
                                            "length_mean", "distance_mean", "distance_max"))
