"""CPU: the raw sums' boundary (wk_ppo_sums, wk_ppo_sums_add, wk_ppo_stats_from_sums,
wk_log_std_grad_from_sums; include/wk_api.h, csrc/wk_sums.cpp) and the record exchange's
declarations -- the structure against the header, ctypes and C#, the three host functions against
tests/sumsref.py byte for byte, the fold's order, the argument errors that need no device, and the
same host code as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sumsref
from test_csharp_binding import cs_struct_layouts
from test_eval_binding import HDR, ROOT, _header_fields

CTYPE = {"int64_t": C.c_int64, "double": C.c_double}


def test_ppo_sums_layout(wk):
    py = wk.PpoSums
    assert wk.PPO_SUMS is py
    assert [(nm, CTYPE[t]) for t, nm in _header_fields("wk_ppo_sums")] == list(py._fields_)
    assert tuple(f for f, _ in py._fields_) == sumsref.FIELDS
    assert C.sizeof(py) == 13 * 8 and [getattr(py, f).offset for f, _ in py._fields_] == [8 * i for i in range(13)]
    lay, size = cs_struct_layouts()["WkPpoSums"]
    assert size == 13 * 8 and [(o, s) for _, o, s in lay] == [(8 * i, 8) for i in range(13)]
    assert [nm.lower() for nm, _, _ in lay] == [f for f, _ in py._fields_]
    assert set(py().as_dict()) == set(sumsref.FIELDS)


def test_record_words_and_declarations(wk):
    assert re.search(r"enum \{ WK_COMM_RECORD_WORDS = 16 \};", HDR) and wk.COMM_RECORD_WORDS == 16
    assert 1 + 13 <= wk.COMM_RECORD_WORDS  # the header word and the widest record
    assert re.search(r"typedef int wk_host_allgather_fn\(const uint64_t\* mine[^;]*uint64_t\* all[^;]*void\* user\);", HDR)
    assert re.search(r"int wk_comm_records\(wk_ctx\* ctx, wk_host_allgather_fn\* fn_or_null, void\* user\);", HDR)
    nat = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "NativeMethods.cs")).read()
    api = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "Api.cs")).read()
    assert "public delegate int HostAllGather(IntPtr mine, IntPtr all, IntPtr user);" in nat
    assert "extern int wk_comm_records(IntPtr ctx, IntPtr fnOrNull, IntPtr user);" in nat
    assert "Marshal.GetFunctionPointerForDelegate(fn)" in nat and "Wk.CommRecords(ctx" in api
    for fn in ("wk_comm_records", "wk_ppo_sums_add", "wk_ppo_stats_from_sums", "wk_log_std_grad_from_sums",
               "wk_policy_sums", "wk_policy_stats_global"):
        assert fn in wk.EXPORTS and hasattr(wk.load_library(), fn)
        assert re.search(r"extern (int|void) %s\(" % fn, nat)
    for fn in ("wk_ppo_sums_add", "wk_ppo_stats_from_sums", "wk_log_std_grad_from_sums", "wk_policy_sums",
               "wk_policy_stats_global"):
        assert "Wk.%s(" % fn in api
    for m in ("comm_records", "policy_sums", "policy_stats_global"):
        assert callable(getattr(wk.Engine, m))
    from wk import dist
    assert callable(dist.gather_records)


def _records():
    rng = np.random.default_rng(20250905)
    return [("random%d" % i, sumsref.random_record(rng)) for i in range(200)] + sorted(sumsref.edge_records().items())


def test_stats_from_sums_is_the_restatement(wk):
    for name, s in _records():
        got, want = wk.stats_from_sums(s), sumsref.stats_from_sums(s)
        assert sumsref.same_bytes(got, want, sumsref.STATS_KEYS), (name, got, want)
    e = sumsref.edge_records()
    g = wk.stats_from_sums(e["no_rows"])
    assert all(np.isnan(g[k]) for k in ("kl", "kl_k1", "clip_fraction", "ratio_max", "surrogate", "value_loss",
                                        "explained_variance")) and g["samples"] == 0
    assert np.isnan(wk.stats_from_sums(e["flat_var"])["explained_variance"])
    assert np.isnan(wk.stats_from_sums(e["nan_srr"])["explained_variance"])
    assert wk.stats_from_sums(e["rmax_none"])["ratio_max"] == -np.inf
    p = wk.stats_from_sums(e["plain"])
    assert p["kl"] == 0.25 / 32 and p["value_loss"] == 0.25 and p["explained_variance"] == 1.0 - (0.25 - 1 / 64) / 1.0


def test_log_std_grad_from_sums_is_the_restatement(wk):
    for coef in (0.0, 0.01, 0.3):
        for name, s in _records():
            got, want = wk.log_std_grad_from_sums(s, coef), sumsref.log_std_grad_from_sums(s, coef)
            assert sumsref.same_bytes(got, want, sumsref.GRAD_KEYS), (name, coef, got, want)
    g = wk.log_std_grad_from_sums(sumsref.edge_records()["no_rows"], 0.01)
    assert np.isnan(g["grad"]) and np.isnan(g["z2_mean"]) and g["samples"] == 0
    g = wk.log_std_grad_from_sums(sumsref.edge_records()["plain"], 0.5)
    assert (g["grad_surrogate"], g["grad"], g["z2_mean"]) == (6.0 / 32, 6.0 / 32 - 0.5, 30.0 / 32)


def test_sums_add_pins_the_order(wk):
    """(1e16 + 1) + 1 == 1e16 in double while 1e16 + (1 + 1) == 1e16 + 2: the fold's order shows"""
    z = sumsref.zero()
    a, b, c = (dict(z, rows=r, kl=v, zz=-v, rmax=m) for r, v, m in ((3, 1e16, 1.5), (5, 1.0, 2.5), (7, 1.0, 0.5)))
    left = wk.sums_add(wk.sums_add(a, b), c)
    right = wk.sums_add(a, wk.sums_add(b, c))
    assert left["kl"] == 1e16 and right["kl"] == 1e16 + 2 and left["zz"] == -1e16 and right["zz"] == -1e16 - 2
    assert left["rows"] == right["rows"] == 15 and left["rmax"] == right["rmax"] == 2.5
    assert sumsref.same_bytes(left, sumsref.fold([a, b, c]), sumsref.FIELDS)
    assert not sumsref.same_bytes(left, sumsref.fold([b, c, a]), sumsref.FIELDS)
    rng = np.random.default_rng(7)
    recs = [sumsref.random_record(rng) for _ in range(40)]
    acc = recs[0]
    for r in recs[1:]:
        acc = wk.sums_add(acc, r)
    assert sumsref.same_bytes(acc, sumsref.fold(recs), sumsref.FIELDS)
    assert sumsref.same_bytes(a, wk.sums_add(a, z), sumsref.FIELDS)  # the record of no rows is the unit


def test_sums_add_keeps_a_nan_rmax_from_either_side(wk):
    z = sumsref.zero()
    nan, five = dict(z, rmax=float("nan")), dict(z, rmax=5.0)
    assert np.isnan(wk.sums_add(nan, five)["rmax"]) and np.isnan(wk.sums_add(five, nan)["rmax"])
    assert np.isnan(sumsref.add(nan, five)["rmax"]) and np.isnan(sumsref.add(five, nan)["rmax"])
    assert wk.sums_add(five, dict(z, rmax=float("inf")))["rmax"] == np.inf
    assert wk.sums_add(z, z)["rmax"] == -np.inf


def test_null_arguments(wk):
    lib = wk.load_library()
    s, st = wk.PpoSums(), wk.PpoStats()
    assert lib.wk_policy_sums(None, C.byref(s), None) == -1
    assert lib.wk_policy_stats_global(None, C.byref(st)) == -1
    assert lib.wk_comm_records(None, None, None) == -1
    lib.wk_ppo_sums_add(None, C.byref(s))  # the context-free functions ignore NULLs
    lib.wk_ppo_stats_from_sums(None, C.byref(st))
    lib.wk_log_std_grad_from_sums(C.byref(s), 0.0, None)


def _host_compiler():
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    return rocm if os.path.exists(rocm) else shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")


def test_host_side_under_sanitizers(tmp_path):
    """tests/cpp/sums_check.cpp: the three host functions on the edge records and the fold's order --
    plain host code with its own main, built with -fsanitize=address,undefined and run as it is"""
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sums_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "sums_check.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "sums_check ok" in r.stdout, r.stdout + r.stderr
