"""CPU: the reward normalisation's boundary (wk_reward_norm_args, wk_reward_norm and the eight
wk_reward_norm_* / wk_get_scaled_rewards entry points; include/wk_api.h) in the mirrors -- the
ctypes structures against the header's layout, the C# structs against the ctypes ones, the C++
and C# object APIs calling the exports -- that wk_config did not grow, and the argument errors
that need no device."""
import ctypes as C
import os
import re

import pytest

from test_csharp_binding import cs_struct_layouts
from test_eval_binding import HDR, ROOT, _header_fields

CTYPE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
STRUCTS = [("wk_reward_norm_args", "RewardNormArgs", "WkRewardNormArgs"), ("wk_reward_norm", "RewardNorm", "WkRewardNorm")]
FUNCS = ("wk_reward_norm_config", "wk_reward_norm_get", "wk_reward_norm_set", "wk_reward_norm_get_acc",
         "wk_reward_norm_set_acc", "wk_reward_norm_update", "wk_get_scaled_rewards")


@pytest.mark.parametrize("c_name,py_name,_", STRUCTS)
def test_ctypes_fields_follow_the_header(wk, c_name, py_name, _):
    py = getattr(wk, py_name)
    assert [(nm, CTYPE[t]) for t, nm in _header_fields(c_name)] == list(py._fields_)


def test_sizes_and_offsets(wk):
    a, s = wk.RewardNormArgs, wk.RewardNorm
    assert (C.sizeof(a), C.sizeof(s)) == (16, 80)
    assert [getattr(a, f).offset for f, _ in a._fields_] == [0, 4, 8, 12]
    assert [getattr(s, f).offset for f, _ in s._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 64, 72]
    assert set(wk.RewardNorm().as_dict()) == {f for f, _ in s._fields_} - {"pad"}
    assert set(wk.RewardNormArgs().as_dict()) == {"enable", "frozen", "clip", "epsilon"}


@pytest.mark.parametrize("_,py_name,cs_name", STRUCTS)
def test_csharp_struct_layouts(wk, _, py_name, cs_name):
    lay, size = cs_struct_layouts()[cs_name]
    py = getattr(wk, py_name)
    assert size == C.sizeof(py)
    assert [(o, s) for _, o, s in lay] == [(getattr(py, f[0]).offset, getattr(py, f[0]).size) for f in py._fields_]
    assert [nm.lower() for nm, _, _ in lay] == [f[0] for f in py._fields_]


def test_wk_config_is_unchanged(wk):
    """the feature is switched on per context at run time: no field in wk_config, its mirrors or
    the JSON document"""
    size = {"int": 4, "float": 4, "char*": 8}
    off = 0
    hdr = _header_fields("wk_config")
    for t, nm in hdr:  # (`const char* Name` parses as ("const", "char*"), ("const", Name): one pointer)
        if nm == "char*":
            continue
        a = 8 if t == "const" else size[t]
        off = (off + a - 1) // a * a + a
    assert (off + 7) // 8 * 8 == 152 == C.sizeof(wk.WkConfigLogStd)
    assert [nm for _, nm in hdr][-5:] == ["LearnLogStd", "LogStdAlpha", "EntropyCoef", "LogStdMin", "LogStdMax"]
    lay, cs_size = cs_struct_layouts()["WkConfigLogStd"]
    assert cs_size == 152
    names = {nm.lower() for _, nm in hdr} | {f[0].lower() for f in wk.WkConfigLogStd._fields_} | {nm.lower() for nm, _, _ in lay}
    assert not any("reward" in nm or "rnorm" in nm for nm in names)
    text = wk.config_to_json(wk.default_config()).lower()
    assert "reward" not in text and "norm" not in text.replace("normalizeadvantages", "")


def test_object_apis_call_the_exports(wk):
    api = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "Api.cs")).read()
    nat = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "NativeMethods.cs")).read()
    nea = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "csrc", "host", "nea.hpp")).read()
    assert re.search(r"void wk_reward_norm_defaults\(wk_reward_norm_args\*", HDR)
    assert "wk_reward_norm_defaults" in wk.EXPORTS and "wk_reward_norm_defaults(ref WkRewardNormArgs" in nat
    assert "Wk.wk_reward_norm_defaults(ref" in api and "wk_reward_norm_defaults(&" in nea
    for fn in FUNCS:
        assert re.search(r"int %s\(wk_ctx\*" % fn, HDR) and fn in wk.EXPORTS
        assert "extern int %s(IntPtr ctx" % fn in nat
        assert "Wk.%s(ctx" % fn in api and "%s(ctx_" % fn in nea
    for m in ("reward_norm", "reward_norm_state", "set_reward_norm_state", "reward_acc", "set_reward_acc",
              "reward_norm_update", "scaled_rewards"):
        assert callable(getattr(wk.Engine, m))


def test_defaults(wk):
    lib = wk.load_library()
    a = wk.RewardNormArgs(7, 7, 0.0, 0.0)
    lib.wk_reward_norm_defaults(C.byref(a))
    assert a.as_dict() == {"enable": 0, "frozen": 0, "clip": 10.0, "epsilon": C.c_float(1e-8).value}
    lib.wk_reward_norm_defaults(None)  # a NULL is ignored


def test_null_arguments_are_argument_errors(wk):
    lib = wk.load_library()
    a = wk.RewardNormArgs()
    buf = (C.c_float * 4)()
    assert lib.wk_reward_norm_config(None, C.byref(a)) == -1
    assert lib.wk_reward_norm_get(None, C.byref(wk.RewardNorm())) == -1
    assert lib.wk_reward_norm_set(None, 0, 0.0, 0.0) == -1
    assert lib.wk_reward_norm_get_acc(None, buf) == -1
    assert lib.wk_reward_norm_set_acc(None, buf) == -1
    assert lib.wk_reward_norm_update(None) == -1
    assert lib.wk_get_scaled_rewards(None, buf) == -1
