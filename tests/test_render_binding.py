"""CPU: the frame renderer's boundary (wk_render_args and the four wk_render* entry points,
include/wk_api.h) in the mirrors -- the ctypes structure against the header's layout, the C# struct
against the ctypes one, the object APIs calling the exports -- wk_render_defaults' values, the
errors that need no device, the host side (argument check and segment plan, csrc/wk_render.h) as a
stand-alone program under the address and undefined-behaviour sanitizers, and the built kernel's
resources."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_csharp_binding import cs_struct_layouts
from test_eval_binding import HDR, ROOT, _header_fields

import renderref

CTYPE = {"int32_t": C.c_int32, "float": C.c_float}
FUNCS = ("wk_render", "wk_render_device", "wk_render_states")
PKG = os.path.join(ROOT, "ppo-bipedalwalker_amd")


def test_ctypes_fields_follow_the_header(wk):
    assert [(nm, CTYPE[t]) for t, nm in _header_fields("wk_render_args")] == list(wk.RenderArgs._fields_)
    a = wk.RenderArgs
    assert C.sizeof(a) == 40 and [getattr(a, f).offset for f, _ in a._fields_] == list(range(0, 40, 4))
    assert set(wk.RenderArgs().as_dict()) == {f for f, _ in a._fields_} - {"pad"} == set(renderref.DEFAULTS)


def test_csharp_struct_layout(wk):
    lay, size = cs_struct_layouts()["WkRenderArgs"]
    py = wk.RenderArgs
    assert size == C.sizeof(py)
    assert [(o, s) for _, o, s in lay] == [(getattr(py, f[0]).offset, getattr(py, f[0]).size) for f in py._fields_]
    assert [nm.lower() for nm, _, _ in lay] == [f[0] for f in py._fields_]


def test_constants(wk):
    got = dict(re.findall(r"WK_RENDER_(MAX_VIEWS|MAX_DIM|MAX_SEGMENTS) = (\d+)", HDR))
    assert {k: int(v) for k, v in got.items()} == {
        "MAX_VIEWS": wk.RENDER_MAX_VIEWS, "MAX_DIM": wk.RENDER_MAX_DIM, "MAX_SEGMENTS": wk.RENDER_MAX_SEGMENTS}
    assert (wk.RENDER_MAX_VIEWS, wk.RENDER_MAX_DIM, wk.RENDER_MAX_SEGMENTS) == (4096, 2048, 160)
    plan = open(os.path.join(PKG, "csrc", "wk_render.h")).read()
    tile = re.search(r"RENDER_TILE_W = (\d+), RENDER_TILE_H = (\d+), RENDER_BLOCK = (\d+)", plan).groups()
    assert tuple(map(int, tile)) == (wk.RENDER_TILE_W, wk.RENDER_TILE_H, 256)
    # the most a view can hold stays under the kernel's list: joints, marker, rough floor, walker, 32 prop vertices
    assert 16 + 1 + 40 + 29 + 32 == 118 <= wk.RENDER_MAX_SEGMENTS <= 256


def test_object_apis_call_the_exports(wk):
    api = open(os.path.join(PKG, "cs", "Api.cs")).read()
    nat = open(os.path.join(PKG, "cs", "NativeMethods.cs")).read()
    assert re.search(r"void wk_render_defaults\(wk_render_args\*", HDR)
    assert "wk_render_defaults" in wk.EXPORTS and "wk_render_defaults(ref WkRenderArgs" in nat
    assert "Wk.wk_render_defaults(ref" in api
    for fn in FUNCS:
        assert re.search(r"int %s\(wk_ctx\* ctx, const wk_render_args\* args" % fn, HDR) and fn in wk.EXPORTS
        assert "extern int %s(IntPtr ctx, ref WkRenderArgs args" % fn in nat
        assert "Wk.%s(ctx, ref args" % fn in api
    for m in ("render", "render_states", "render_device"):
        assert callable(getattr(wk.Engine, m))


def test_defaults(wk):
    lib = wk.load_library()
    a = wk.RenderArgs(7, 7, 7.0, 7.0, 7.0, 7, 7.0, 7.0, 7, 7)
    lib.wk_render_defaults(C.byref(a))
    d = a.as_dict()
    assert math.isnan(d.pop("marker_x")) and a.pad == 0
    assert d == {"width": 550, "height": 325, "scale": 0.5, "ox": -50.0, "oy": 400.0, "follow": 0,
                 "line_px": 1.0, "joints": 1}
    ref = dict(renderref.DEFAULTS)
    assert math.isnan(ref.pop("marker_x")) and ref == d
    lib.wk_render_defaults(None)  # a NULL is ignored
    # the window is 1100 x 650 world units: the whole flat floor (-50..1050) and the walker
    assert (a.width / a.scale, a.height / a.scale) == (1100.0, 650.0)
    assert wk.render_args(width=96, follow=1).as_dict()["width"] == 96
    with pytest.raises(KeyError):
        wk.render_args(pad=1)


def test_null_context_is_an_argument_error(wk):
    lib = wk.load_library()
    a, ids, img = wk.render_args(), (C.c_int32 * 1)(0), (C.c_uint8 * 4)(1, 2, 3, 4)
    st = (C.c_float * wk.STATE_FLOATS)()
    assert lib.wk_render(None, C.byref(a), ids, 1, img) == -1
    assert lib.wk_render_device(None, C.byref(a), ids, 1, img) == -1
    assert lib.wk_render_states(None, C.byref(a), st, ids, 1, img) == -1
    assert list(img) == [1, 2, 3, 4]


def _host_compiler():
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    return rocm if os.path.exists(rocm) else shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")


def test_host_side_under_sanitizers(tmp_path):
    """tests/cpp/render_plan_check.cpp: defaults, every argument error, the plan's bookkeeping --
    plain host code with its own main, built with -fsanitize=address,undefined and run as it is"""
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "render_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "render_plan_check.cpp"),
                    "-o", exe], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "render_plan_check ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/llvm/bin/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
def test_render_kernel_resources(wk):
    """no scratch, no spill, and at most 64 VGPRs (the build has 46): eight waves per SIMD stay
    resident"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    res = {k: v for k, v in kernel_resources(wk.LIB_PATH).items() if "k_render" in k}
    assert len(res) == 1, sorted(res)
    (scratch, spilled, vgprs), = res.values()
    assert scratch == 0 and spilled == 0 and vgprs <= 64, res
