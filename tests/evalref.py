"""Reference for wk_evaluate: the episode end-kind rule, a float64 aggregation of episode
records, and oracle-driven complete episodes.  Test infrastructure only (no GPU)."""
import math

import numpy as np

FELL, TIME_LIMIT, SUCCESS, UNFINISHED = 0, 1, 2, 3
REC_DTYPE = np.dtype([("total_reward", np.float32), ("length", np.int32), ("distance", np.float32),
                      ("final_x", np.float32), ("end", np.int32), ("env", np.int32)])

# the CPU case the GPU emulation test shares: 24 walkers at the RandomizeStart offsets of the
# seed, walker 3 moved next to the goal (its first step succeeds), a short time limit and random
# weights under which some walkers fall and some last
CASE_N, CASE_MT, CASE_EPISODES, CASE_WEIGHT_SEED, CASE_GOAL_WALKER, CASE_GOAL_DX = 24, 120, 2, 4, 3, 780.0


def case_offsets(orc, seed, n=CASE_N):
    dx = np.array([orc.env_offset(seed, i) for i in range(n)], np.float32)
    dx[CASE_GOAL_WALKER] = CASE_GOAL_DX
    return dx


def case_weights(weight_seed=CASE_WEIGHT_SEED, nparam=6149):
    return np.random.default_rng(weight_seed).normal(0, 0.5, nparam).astype(np.float32)


def end_kind(final_x, length, max_timesteps):
    """what the physics emits decides: past the goal line, else past the time limit, else a fall
    (a fall on the very step of the limit counts as the limit)"""
    if np.float32(final_x) > np.float32(900.0):
        return SUCCESS
    if int(length) > int(max_timesteps):
        return TIME_LIMIT
    return FELL


class Running:
    """one walker's episode accounting, as the evaluation keeps it: a double reward sum rounded
    once, the length, the largest x (NaN ignored) and the last x"""

    def __init__(self, env, episodes, max_timesteps):
        self.env, self.episodes, self.mt = env, episodes, max_timesteps
        self.recs = []
        self._start()

    def _start(self):
        self.acc, self.len, self.best = 0.0, 0, np.float32(-np.inf)

    def done(self):
        return len(self.recs) >= self.episodes

    def add(self, reward, done, x):
        if self.done():
            return
        self.acc += float(np.float32(reward))
        self.len += 1
        x = np.float32(x)
        if x > self.best:
            self.best = x
        if done:
            self.recs.append((np.float32(self.acc), self.len, self.best, x,
                              end_kind(x, self.len, self.mt), self.env))
            self._start()


def records_array(runs, episodes):
    """[episodes][n] records from per-walker Running objects; unfinished slots are UNFINISHED and
    zero otherwise"""
    out = np.zeros((episodes, len(runs)), REC_DTYPE)
    out["end"] = UNFINISHED
    for e, r in enumerate(runs):
        for k, rec in enumerate(r.recs):
            out[k, e] = rec
    return out


def oracle_episodes(orc, dx, weights, episodes, max_timesteps, max_steps=None):
    """every walker plays `episodes` complete episodes under Agent.mean on the oracle, from
    Env.reset().  Returns (records [episodes][n], the env-steps the slowest walker needed)"""
    ag = orc.Agent()
    ag.set_params(weights)
    runs, needed = [], 0
    cap = episodes * (max_timesteps + 1) if max_steps is None else max_steps
    for i, d in enumerate(dx):
        env = orc.Env(dx=float(d), MaxTimesteps=max_timesteps)
        env.reset()
        run, obs, t = Running(i, episodes, max_timesteps), env.obs(), 0
        while not run.done() and t < cap:
            obs, r, dn = env.step(ag.mean(obs))
            run.add(r, dn, env.step_position()[0])
            t += 1
        runs.append(run)
        needed = max(needed, t)
    return records_array(runs, episodes), needed


def aggregate(recs):
    """float64 statistics of the finished records, with wk_eval_stats' names (exactly rounded
    sums: math.fsum)"""
    r = np.asarray(recs).reshape(-1)
    fin = r[r["end"] != UNFINISHED]
    c = len(fin)
    out = dict(episodes=c, unfinished=len(r) - c, fell=int((fin["end"] == FELL).sum()),
               timed_out=int((fin["end"] == TIME_LIMIT).sum()),
               succeeded=int((fin["end"] == SUCCESS).sum()))
    nan = float("nan")
    if c == 0:
        out.update(reward_mean=nan, reward_std=nan, reward_min=nan, reward_max=nan, length_mean=nan,
                   length_min=0, length_max=0, distance_mean=nan, distance_max=nan)
        return out
    x = [float(v) for v in fin["total_reward"]]
    d = [float(v) for v in fin["distance"]]
    mean = math.fsum(x) / c
    out.update(reward_mean=mean,
               reward_std=math.sqrt(max(0.0, math.fsum(v * v for v in x) / c - mean * mean)),
               reward_min=min(x), reward_max=max(x),
               length_mean=int(fin["length"].astype(np.int64).sum()) / c,
               length_min=int(fin["length"].min()), length_max=int(fin["length"].max()),
               distance_mean=math.fsum(d) / c, distance_max=max(d))
    return out


def sum_bound(values, n=None):
    """the bound of an ordered double sum of `values` against the exactly rounded one:
    4 N 2^-53 sum|x| (each of the N - 1 additions rounds to 2^-53 of a partial sum that is at
    most sum|x|; the factor 4 covers the regrouping into lane, wave and block sums)"""
    v = [abs(float(x)) for x in values]
    return 4.0 * (len(v) if n is None else n) * 2.0 ** -53 * math.fsum(v)
