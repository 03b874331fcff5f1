"""CPU: the log-std's boundary (LearnLogStd and its config fields, wk_get / wk_set_log_std,
wk_set_log_std_adam, wk_log_std_gradient; include/wk_api.h) in the mirrors -- the ctypes
structures against the header's layout, the C# structs against the ctypes ones, the C++ and C#
object APIs calling the exports -- and the argument errors that need no device."""
import ctypes as C
import os
import re

import pytest

from test_csharp_binding import cs_struct_layouts
from test_eval_binding import HDR, ROOT, _header_fields

CTYPE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
STRUCTS = [("wk_log_std_grad", "LogStdGrad", "WkLogStdGrad"), ("wk_log_std_state", "LogStdState", "WkLogStdState")]
CONFIG = [("int", "LearnLogStd"), ("float", "LogStdAlpha"), ("float", "EntropyCoef"), ("float", "LogStdMin"),
          ("float", "LogStdMax")]


@pytest.mark.parametrize("c_name,py_name,_", STRUCTS)
def test_ctypes_fields_follow_the_header(wk, c_name, py_name, _):
    py = getattr(wk, py_name)
    assert [(nm, CTYPE[t]) for t, nm in _header_fields(c_name)] == list(py._fields_)


def test_sizes_and_offsets(wk):
    g, s = wk.LogStdGrad, wk.LogStdState
    assert (C.sizeof(g), C.sizeof(s)) == (40, 72)
    assert [getattr(g, f).offset for f, _ in g._fields_] == [0, 8, 16, 24, 32]
    assert [getattr(s, f).offset for f, _ in s._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert set(wk.LogStdState().as_dict()) == {f for f, _ in s._fields_} - {"pad"}


def test_config_fields(wk):
    """the five fields, appended at the end of wk_config in the header's order, with the header's
    defaults; none of them is part of the JSON document"""
    hdr = _header_fields("wk_config")
    assert hdr[-5:] == CONFIG
    # the ctypes mirror of the whole struct is WkConfigLogStd: WkConfig (the fields up to
    # MaxGradNorm, as before) and the five appended by subclassing
    full = wk.WkConfigLogStd
    assert issubclass(full, wk.WkConfig) and list(full._fields_) == [(nm, CTYPE[t]) for t, nm in CONFIG]
    # (the two `const char* Name` declarations parse as the names "char*" and Name)
    assert [nm for _, nm in hdr if nm != "char*"] == [f[0] for f in wk.WkConfig._fields_] + [f[0] for f in full._fields_]
    off = full.MaxGradNorm.offset + 4
    assert off == C.sizeof(wk.WkConfig)  # no tail padding in the base: the C struct's offsets
    assert [getattr(full, nm).offset for _, nm in CONFIG] == [off + 4 * i for i in range(5)]
    assert C.sizeof(full) == (off + 20 + 7) // 8 * 8 == 152
    for nm, _ in wk.WkConfig._fields_:
        assert getattr(full, nm).offset == getattr(wk.WkConfig, nm).offset
    c = wk.default_config()
    assert type(c) is full
    # the library takes the whole struct only: the 128-byte head is refused by the signature
    with pytest.raises(C.ArgumentError):
        wk.load_library().wk_config_defaults(C.byref(wk.WkConfig()))
    assert (c.LearnLogStd, c.LogStdAlpha, c.EntropyCoef, c.LogStdMin, c.LogStdMax) == (0, 0.0, 0.0, -4.0, 1.0)
    text = wk.config_to_json(wk.default_config(LearnLogStd=1, EntropyCoef=0.5))
    assert not any(nm in text for _, nm in CONFIG)


@pytest.mark.parametrize("_,py_name,cs_name", STRUCTS)
def test_csharp_struct_layouts(wk, _, py_name, cs_name):
    lay, size = cs_struct_layouts()[cs_name]
    py = getattr(wk, py_name)
    assert size == C.sizeof(py)
    assert [(o, s) for _, o, s in lay] == [(getattr(py, f[0]).offset, getattr(py, f[0]).size) for f in py._fields_]


def test_csharp_config(wk):
    """C#'s WkConfigLogStd is the whole wk_config, field for field the ctypes one, and every
    import that takes a wk_config takes it"""
    lay, size = cs_struct_layouts()["WkConfigLogStd"]
    full = wk.WkConfigLogStd
    names = [f[0] for f in wk.WkConfig._fields_] + [f[0] for f in full._fields_]
    assert size == C.sizeof(full)
    assert lay == [(nm, getattr(full, nm).offset, getattr(full, nm).size) for nm in names]
    cs = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "NativeMethods.cs")).read()
    assert "ref WkConfig cfg" not in cs and cs.count("ref WkConfigLogStd cfg") == 6


def test_object_apis_call_the_exports(wk):
    api = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "cs", "Api.cs")).read()
    nea = open(os.path.join(ROOT, "ppo-bipedalwalker_amd", "csrc", "host", "nea.hpp")).read()
    for fn in ("wk_get_log_std", "wk_set_log_std", "wk_set_log_std_adam", "wk_log_std_gradient"):
        assert re.search(r"int %s\(wk_ctx\*" % fn, HDR) and fn in wk.EXPORTS
        assert "Wk.%s(ctx" % fn in api and "%s(ctx_" % fn in nea
    for m in ("log_std", "set_log_std", "set_log_std_adam", "log_std_gradient"):
        assert callable(getattr(wk.Engine, m))


def test_null_context_is_an_argument_error(wk):
    lib = wk.load_library()
    assert lib.wk_get_log_std(None, C.byref(wk.LogStdState())) == -1
    assert lib.wk_set_log_std(None, -1.0) == -1
    assert lib.wk_set_log_std_adam(None, 0.0, 0.0, 0) == -1
    assert lib.wk_log_std_gradient(None, C.byref(wk.LogStdGrad())) == -1
