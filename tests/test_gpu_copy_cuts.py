"""GPU: the rollout's copy cuts move data and operands only, so each is checked bit for bit on
the device against the form it replaces (stand-alone programs built by the Makefile's `check`
target, like tests/cpp/floor_face_check.hip):

- the rotation's Horner steps as three-address FMAs with scalar constants against the same
  thirteen FMAs written with __builtin_fma (tests/cpp/sincos_dev_check.hip);
- the contact faces through the LDS column's one-word planes against the register form, both
  instantiations of the contact points on the same inputs, and the legs' park / unpark in the
  same planes while other waves write face records (tests/cpp/face_lds_check.hip).
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppo-bipedalwalker_amd")


def _run_check(name, timeout):
    exe = os.path.join(PKG, "build", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", PKG, "check"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    return r.stdout


def test_sincos_small_device_form():
    """wk_sincos_small as the device build compiles it equals the plain FMA restatement: both
    doubles and both (float) results bit for bit, for every float with |a| <= 0.25 and 8,192
    hashed floats outside it."""
    out = _run_check("sincos_dev_check", 120)
    assert "2097152002 floats" in out  # 2 (0x3e800000 + 1): every float of the range, both signs


def test_face_column_planes():
    """significant_face_lds in the planes layout equals significant_face_ax (fa, fb, fmax, fdir,
    NaN normals included), contact_points_ax / contact_points_floor agree between S > 0 and
    S = 0, and parked legs survive other waves' face records: 1,048,576 cases."""
    out = _run_check("face_lds_check", 120)
    assert "1048576 cases" in out
