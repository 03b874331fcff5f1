"""CPU: the evaluation's boundary (wk_evaluate, include/wk_api.h) in the three mirrors -- the ctypes
structures against the header's layout, the C# structs against the ctypes ones, the C++ and C#
object APIs calling the export -- and the argument errors that need no device."""
import ctypes as C
import os
import re

import pytest

from test_csharp_binding import cs_struct_layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "wk_api.h")).read()


def test_header_constants_match_python(wk):
    assert int(re.search(r"WK_EVAL_MAX_EPISODES = (\d+)", HDR).group(1)) == wk.EVAL_MAX_EPISODES == 16
    ends = dict(re.findall(r"WK_EVAL_(FELL|TIME_LIMIT|SUCCESS|UNFINISHED) = (\d)", HDR))
    assert {k: int(v) for k, v in ends.items()} == {
        "FELL": wk.EVAL_FELL, "TIME_LIMIT": wk.EVAL_TIME_LIMIT, "SUCCESS": wk.EVAL_SUCCESS,
        "UNFINISHED": wk.EVAL_UNFINISHED}
    import evalref
    assert (evalref.FELL, evalref.TIME_LIMIT, evalref.SUCCESS, evalref.UNFINISHED) == (0, 1, 2, 3)
    assert evalref.REC_DTYPE == wk.EVAL_DTYPE


def _header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HDR, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        toks = decl.replace(",", " ").split()
        if toks:
            out += [(toks[0], nm) for nm in toks[1:]]
    return out


@pytest.mark.parametrize("c_name,py_name", [("wk_eval_args", "EvalArgs"), ("wk_eval_rec", "EvalRec"),
                                            ("wk_eval_stats", "EvalStats")])
def test_ctypes_fields_follow_the_header(wk, c_name, py_name):
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float,
             "double": C.c_double}
    py = getattr(wk, py_name)
    assert [(nm, ctype[t]) for t, nm in _header_fields(c_name)] == list(py._fields_)


def test_sizes(wk):
    assert (C.sizeof(wk.EvalArgs), C.sizeof(wk.EvalRec), C.sizeof(wk.EvalStats)) == (24, 24, 120)
    assert wk.EVAL_DTYPE.itemsize == C.sizeof(wk.EvalRec)


@pytest.mark.parametrize("cs_name,py_name", [("WkEvalArgs", "EvalArgs"), ("WkEvalRec", "EvalRec"),
                                             ("WkEvalStats", "EvalStats")])
def test_csharp_struct_layouts(wk, cs_name, py_name):
    lay, size = cs_struct_layouts()[cs_name]
    py = getattr(wk, py_name)
    assert size == C.sizeof(py)
    assert [(o, s) for _, o, s in lay] == [(getattr(py, f[0]).offset, getattr(py, f[0]).size) for f in py._fields_]


def test_object_apis_call_the_export():
    api = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "Api.cs")).read()
    nea = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "csrc", "host", "nea.hpp")).read()
    assert "Wk.wk_evaluate(ctx, ref args, out var s, records)" in api
    assert "wk_eval_stats Evaluate(" in nea and "wk_evaluate(ctx_, &args, &s," in nea


def test_null_context_is_an_argument_error(wk):
    lib = wk.load_library()
    st = wk.EvalStats()
    assert lib.wk_evaluate(None, None, C.byref(st), None) == -1
    s, f = C.c_double(), C.c_double()
    assert lib.wk_evaluate_time(None, 4, C.byref(s), C.byref(f)) == -1
