"""CPU: the general networks' host side (NetworkKernels = 1) -- the network-string parser and its
limits (csrc/wk_net.h), wk_net_param_count, wk_create's refusals before any device is touched,
the weights text conversion for any pair of strings, and the general kernels' resources."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import netref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppo-bipedalwalker_amd")
LIB = os.path.join(PKG, "libwk.so")
F = np.float32

CD, AD = netref.CRITIC_DEFAULT, netref.ACTOR_DEFAULT


def test_param_counts(wk):
    assert wk.net_param_count() == (897, 5252) == wk.net_param_count(CD, AD)
    assert wk.net_param_count(*netref.NETS["tiny"]) == (13, 52)
    assert sum(wk.net_param_count(*netref.NETS["max"])) == 70021
    for name, (c, a) in netref.NETS.items():
        assert wk.net_param_count(c, a) == (netref.n_params(c), netref.n_params(a)), name


@pytest.mark.parametrize("critic,actor,msg", [
    ("Input |129| (ReLU) |1| Output", AD, "width"),                       # a width over 128
    (CD, "Input |8| |8| |8| |8| |4| Output", "dense"),                     # 5 dense layers
    (CD, "Input |8| (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) |4| Output", "layers"),  # 9 layers
    ("Input |0| |1| Output", AD, "not valid"),
    (CD, "Input |64| (LeakyReLU) |3| Output", "should output 4"),
    (CD, "Input |64| (Sigmoid) |4| Output", "not valid"),
])
def test_param_count_refuses(wk, critic, actor, msg):
    lib = wk.load_library()
    nc, na = C.c_int(-1), C.c_int(-1)
    rc = lib.wk_net_param_count(critic.encode(), actor.encode(), C.byref(nc), C.byref(na))
    assert rc == -3  # WK_ERR_CONFIG
    assert msg in lib.wk_last_error(None).decode()
    with pytest.raises(wk.WkError):
        wk.net_param_count(critic, actor)


def _create(wk, **cfg):
    lib = wk.load_library()
    c = wk.default_config(**cfg)
    h = C.c_void_p()
    rc = lib.wk_create(C.byref(c), 0, 8, 1, C.byref(h))
    msg = lib.wk_last_error(None).decode()
    if rc == 0:
        lib.wk_destroy(h)
    return rc, msg


def test_create_accepts_general_networks(wk):
    """with NetworkKernels = 1 a valid string within the limits passes the configuration check
    (without a device the create then fails at the device, -2)"""
    assert wk.default_config().NetworkKernels == 0
    for name, (c, a) in netref.NETS.items():
        rc, msg = _create(wk, NetworkKernels=1, CriticNeuralNetwork=c, ActorNeuralNetwork=a)
        assert rc in (0, -2), (name, rc, msg)
    rc, msg = _create(wk, NetworkKernels=1)  # the default strings on the general kernels
    assert rc in (0, -2), msg


def test_create_refuses_over_limit_before_the_device(wk):
    rc, msg = _create(wk, NetworkKernels=1, CriticNeuralNetwork="Input |200| |1| Output")
    assert rc == -3 and "width" in msg and "200" in msg
    rc, msg = _create(wk, NetworkKernels=1, ActorNeuralNetwork="Input |8| |8| |8| |8| |4| Output")
    assert rc == -3 and "dense" in msg
    rc, msg = _create(wk, NetworkKernels=1, ActorNeuralNetwork="Input |4| (Sigmoid) Output")
    assert rc == -3 and "actor network" in msg
    rc, msg = _create(wk, NetworkKernels=2)
    assert rc == -3 and "NetworkKernels" in msg


def test_create_without_the_switch_refuses_as_before(wk):
    c, a = netref.NETS["odd"]
    rc, msg = _create(wk, ActorNeuralNetwork=a)
    assert rc == -3 and "unsupported" in msg and "actor network" in msg and "NetworkKernels" in msg
    rc, msg = _create(wk, CriticNeuralNetwork=c)
    assert rc == -3 and "unsupported" in msg and "critic network" in msg


@pytest.mark.parametrize("name", ["odd", "max", "tiny", "default"])
def test_weights_text_round_trip(wk, name):
    c, a = netref.NETS[name]
    n = sum(wk.net_param_count(c, a))
    rng = np.random.default_rng(len(name))
    p = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-12, 12, n)).astype(F)
    p[:3] = [0.0, -0.0, np.inf]
    ct, at = wk.format_weights(p, c, a)
    assert ct.split("\n")[0] == c and at.split("\n")[0] == a
    assert len(ct.strip().split("\n")) == 1 + sum(1 for l in netref.layers(c) if l[0] == "D")
    q = wk.parse_weights(ct, at, c, a)
    assert q.view(np.uint32).tolist() == p.view(np.uint32).tolist()  # bit for bit
    # a text whose line 0 is another string is refused
    other = ct.replace(c, "Input |2| |1| Output", 1)
    with pytest.raises(wk.WkError, match="does not match"):
        wk.parse_weights(other, at, c, a)
    if name != "default":
        with pytest.raises(wk.WkError):
            wk.parse_weights(ct, at)  # the default strings' parser


def test_default_text_is_the_same_through_both_entries(wk):
    p = np.random.default_rng(3).normal(0, 1, wk.NPARAM).astype(F)
    assert wk.format_weights(p) == wk.format_weights(p, CD, AD)
    lib = wk.load_library()
    need = -lib.wk_format_weights(p.ctypes.data, None, 0, None, 0)
    cb, ab = C.create_string_buffer(need), C.create_string_buffer(need)
    assert lib.wk_format_weights(p.ctypes.data, cb, need, ab, need) == 0
    assert (cb.value.decode(), ab.value.decode()) == wk.format_weights(p)


def test_parser_under_sanitizers(tmp_path):
    """tests/cpp/net_spec_check.cpp: the parser on the test networks, every truncation of the
    default strings, empty and very long input, built with AddressSanitizer + UBSan (host code,
    its own main; the runtimes linked statically, so the program runs as it is)"""
    exe = str(tmp_path / "net_spec_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    f"-I{os.path.join(PKG, 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "net_spec_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "net_spec_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/llvm/bin/clang-offload-bundler"),
                    reason="needs the built libwk.so and the ROCm LLVM tools")
def test_general_kernels_have_no_scratch():
    """accumulators and fragments are indexed with constants only: nothing of k_net_grad or
    k_net_policy (every instantiation) lands in scratch"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    res = kernel_resources(LIB)
    net = {k: v for k, v in res.items() if "k_net_grad" in k or "k_net_policy" in k}
    assert any("k_net_grad" in k for k in net) and any("k_net_policy" in k for k in net), sorted(net)
    for k, (scratch, spilled, vgprs) in net.items():
        assert scratch == 0 and spilled == 0, (k, scratch, spilled)
