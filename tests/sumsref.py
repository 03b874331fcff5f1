"""numpy-double restatement of the host arithmetic on wk_ppo_sums (include/wk_api.h;
csrc/wk_sums.cpp): the fold step of the record exchange and the two divisions that turn the raw
sums into wk_ppo_stats and wk_log_std_grad -- test infrastructure only.  Every operation is one
IEEE double operation in the order the C++ writes it, so the results compare byte for byte."""
import numpy as np

D = np.float64
INT_FIELDS = ("rows", "skipped", "clipped")
DBL_FIELDS = ("kl", "k1", "surr", "sr", "srr", "se", "see", "rmax", "term", "zz")
FIELDS = INT_FIELDS + DBL_FIELDS  # the header's order: 13 64-bit words
STATS_KEYS = ("samples", "skipped", "kl", "kl_k1", "clip_fraction", "ratio_max", "surrogate", "value_loss",
              "explained_variance", "epochs_run", "stopped_early")
GRAD_KEYS = ("samples", "skipped", "grad_surrogate", "grad", "z2_mean")


def zero():
    """the record of no rows: zero sums, rmax -inf"""
    s = {k: 0 for k in INT_FIELDS}
    s.update({k: 0.0 for k in DBL_FIELDS})
    s["rmax"] = float("-inf")
    return s


def add(acc, x):
    """acc + x: integers add, doubles add, rmax the larger with a NaN on either side staying"""
    out = {k: int(acc[k]) + int(x[k]) for k in INT_FIELDS}
    with np.errstate(all="ignore"):
        for k in DBL_FIELDS:
            out[k] = float(D(acc[k]) + D(x[k]))
    a, b = float(acc["rmax"]), float(x["rmax"])
    out["rmax"] = b if (b > a or b != b) else a
    return out


def fold(records):
    """the exchange's fold: rank 0's record, then the others added in rank order"""
    acc = dict(records[0])
    for r in records[1:]:
        acc = add(acc, r)
    return acc


def stats_from_sums(s):
    """stats_from_rec in numpy doubles"""
    nan = float("nan")
    with np.errstate(all="ignore"):
        n = D(s["rows"])
        ne = D(4.0) * n
        out = dict(samples=int(s["rows"]), skipped=int(s["skipped"]))
        out["kl"] = float(D(s["kl"]) / ne)
        out["kl_k1"] = float(D(s["k1"]) / ne)
        out["clip_fraction"] = float(D(s["clipped"]) / ne)
        out["ratio_max"] = float(s["rmax"]) if s["rows"] > 0 else nan
        out["surrogate"] = float(D(s["surr"]) / ne)
        out["value_loss"] = float(D(s["see"]) / n)
        mr, me = D(s["sr"]) / n, D(s["se"]) / n
        var_r = D(s["srr"]) / n - mr * mr
        var_e = D(s["see"]) / n - me * me
        flat = bool(var_r <= D(4.0) * n * D(2.0 ** -53) * (D(s["srr"]) / n))
        ev = float(D(1.0) - var_e / var_r) if (s["rows"] > 0 and not flat) else nan
        if var_r != var_r:
            ev = nan
        out["explained_variance"] = ev
    out["epochs_run"] = out["stopped_early"] = 0
    return out


def log_std_grad_from_sums(s, entropy_coef):
    """the log-std pass's division; entropy_coef is the fp32 configuration value"""
    with np.errstate(all="ignore"):
        ne = D(4.0) * D(s["rows"])
        gs = -D(s["term"]) / ne
        return dict(samples=int(s["rows"]), skipped=int(s["skipped"]), grad_surrogate=float(gs),
                    grad=float(gs - D(np.float32(entropy_coef))), z2_mean=float(D(s["zz"]) / ne))


def same_bytes(a, b, keys):
    """every value equal as bytes (NaN payloads included for the doubles)"""
    pack = lambda d: b"".join(np.array([d[k]], np.int64 if isinstance(d[k], (int, np.integer)) else D).tobytes()
                              for k in keys)
    return pack(a) == pack(b)


def random_record(rng):
    """a plausible record: counts, sums of both signs"""
    rows = int(rng.integers(1, 1 << 20))
    s = dict(rows=rows, skipped=int(rng.integers(0, 1000)), clipped=int(rng.integers(0, 4 * rows)))
    for k in ("kl", "srr", "see", "zz"):
        s[k] = float(rng.uniform(0, 10) * rows)
    for k in ("k1", "surr", "sr", "se", "term"):
        s[k] = float(rng.normal(0, 3) * rows)
    s["srr"] += s["sr"] * s["sr"] / rows  # (a variance that is not negative)
    s["rmax"] = float(rng.uniform(0.5, 40))
    return s


def edge_records():
    """name -> record: the cases the divisions branch on"""
    nan, inf = float("nan"), float("inf")
    base = dict(rows=8, skipped=1, clipped=5, kl=0.25, k1=-0.5, surr=3.0, sr=16.0, srr=40.0, se=1.0, see=2.0,
                rmax=1.75, term=-6.0, zz=30.0)
    out = {"no_rows": zero(), "plain": base}
    out["flat_var"] = dict(base, sr=24.0, srr=72.0)          # ret = 3 on every row: Var(ret) = 0
    out["nan_srr"] = dict(base, srr=nan)
    out["rmax_none"] = dict(base, rmax=-inf)
    out["rmax_nan"] = dict(base, rmax=nan)
    out["inf_term"] = dict(base, term=inf, zz=inf)
    out["skipped_only"] = dict(zero(), skipped=12)
    return out
