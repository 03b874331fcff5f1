"""Static count of the instructions that do no arithmetic in the rollout's substep loop (CPU only).

Compiles wk_env_pair.hip (the pair side kernels) to gfx950 assembly with the Makefile's own
flags for it (target build/wk_env_pair.hip.s), finds the substep loop of every k_env_side
instantiation -- the innermost loop that holds the rotations' double-precision FMA chains --
and prints per loop: instructions, VALU, register-to-register copies (v_mov_b32 / v_mov_b64
from a VGPR), s_nop count and wait states, and the basic blocks with the most of them.

  python scripts/isa_overhead.py [--asm FILE.s] [--kernel SUBSTRING] [--top N]

`loop_stats(asm_text, kernel_substring)` is the importable form (tests/test_isa_overhead.py).
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppo-bipedalwalker_amd")
ASM_TARGET = os.path.join("build", "wk_env_pair.hip.s")
HEADLINE = "_ZN2wk10k_env_sideILb1ELb1ELb0ELi1ELb0EEEvNS_9EnvParamsENS_8StepArgsE"

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)")
_F64_FMA = ("v_fma_f64", "v_fmac_f64")


def build_asm(jobs=1):
    """The assembly of wk_env_pair.hip, built by the Makefile with that unit's flags."""
    subprocess.run(["make", "-s", "-C", PKG, "-j", str(jobs), ASM_TARGET], check=True)
    return os.path.join(PKG, ASM_TARGET)


def _functions(text, key):
    """(name, body lines) of every kernel whose mangled name holds `key`."""
    out = []
    for m in re.finditer(r"^(_Z\w+):\s*(?:;.*)?$", text, re.M):
        name = m.group(1)
        if key not in name:
            continue
        end = text.find(".Lfunc_end", m.end())
        out.append((name, text[m.end():end].split("\n")))
    return out


def _is_copy(ins):
    """v_mov_b32 / v_mov_b64 from a VGPR (not the DPP / SDWA lane exchanges, not a constant)."""
    parts = ins.replace(",", " ").split()
    if parts[0] not in ("v_mov_b32_e32", "v_mov_b32_e64", "v_mov_b32", "v_mov_b64_e32",
                        "v_mov_b64_e64", "v_mov_b64"):
        return False
    return len(parts) >= 3 and parts[2].startswith("v")


def _stream(lines):
    """[(block label, instruction text)] in program order, and label -> first index."""
    stream, first = [], {}
    block = "entry"
    for raw in lines:
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = _LABEL.match(line)
        if m:
            block = m.group(1)
            first[block] = len(stream)
            continue
        if line.startswith(".") or line.endswith(":"):
            continue
        stream.append((block, line))
    return stream, first


def _count(stream):
    c = {"total": len(stream), "valu": 0, "salu": 0, "lds": 0, "lane_moves": 0, "copies": 0,
         "nops": 0, "wait_states": 0}
    for _, ins in stream:
        op = ins.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
        if op.startswith("s_") and op != "s_nop":
            c["salu"] += 1  # (scalar ALU, branches and waits)
        if op.startswith("ds_"):
            c["lds"] += 1
        if op.startswith(("v_readlane", "v_writelane")):
            c["lane_moves"] += 1  # (scalar registers kept in a VGPR's lanes)
        if _is_copy(ins):
            c["copies"] += 1
        if op == "s_nop":
            c["nops"] += 1
            c["wait_states"] += int(ins.split()[1], 0) + 1
    return c


def loop_stats(text, key="k_env_side"):
    """{kernel: {'total', 'valu', 'copies', 'nops', 'wait_states', 'blocks', 'scratch'}} for the
    substep loop of every kernel whose name holds `key`.  'blocks': [(label, size, copies, nops)]
    sorted by copies + nops; 'scratch': the kernel's .private_segment_fixed_size."""
    res = {}
    for name, lines in _functions(text, key):
        stream, first = _stream(lines)
        loops = []  # (start, end) of every backward branch's range
        for i, (_, ins) in enumerate(stream):
            m = _BRANCH.match(ins)
            if m and m.group(1) in first and first[m.group(1)] <= i:
                loops.append((first[m.group(1)], i + 1))
        fma = [sum(1 for _, ins in stream[a:b] if ins.split()[0].startswith(_F64_FMA)) for a, b in loops]
        if not loops or max(fma) == 0:
            continue
        # the innermost loop with (nearly) all of the chains: the rotations' 15 FMAs each
        a, b = min((l for l, f in zip(loops, fma) if 10 * f >= 9 * max(fma)), key=lambda l: l[1] - l[0])
        body = stream[a:b]
        c = _count(body)
        blocks = {}
        for blk, ins in body:
            e = blocks.setdefault(blk, [0, 0, 0])
            e[0] += 1
            e[1] += _is_copy(ins)
            e[2] += ins.split()[0] == "s_nop"
        c["blocks"] = sorted(((k, v[0], v[1], v[2]) for k, v in blocks.items()),
                             key=lambda t: -(t[2] + t[3]))
        m = re.search(r"\.amdhsa_kernel %s\b.*?\.amdhsa_private_segment_fixed_size (\d+)" % re.escape(name),
                      text, re.S)
        c["scratch"] = int(m.group(1)) if m else None
        res[name] = c
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="an existing assembly file (default: build it)")
    ap.add_argument("--kernel", default="k_env_side", help="substring of the mangled kernel name")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--jobs", type=int, default=1)
    a = ap.parse_args()
    path = a.asm or build_asm(a.jobs)
    res = loop_stats(open(path).read(), a.kernel)
    if not res:
        sys.exit("no kernel with a substep loop matches %r" % a.kernel)
    for name, c in res.items():
        over = c["copies"] + c["nops"]
        print(name + (" (headline)" if name == HEADLINE else ""))
        print("  substep loop: %d instructions, %d VALU, %d copies, %d s_nop (%d wait states), "
              "copies + nops %.1f %% of the stream, scratch %s bytes"
              % (c["total"], c["valu"], c["copies"], c["nops"], c["wait_states"],
                 100.0 * over / c["total"], c["scratch"]))
        print("  of the rest: %d scalar, %d LDS; %d of the VALU move a scalar register to / from a lane"
              % (c["salu"], c["lds"], c["lane_moves"]))
        print("  block        size  copies  nops")
        for blk, size, cp, nop in c["blocks"][:a.top]:
            print("  %-12s %4d  %6d  %4d" % (blk, size, cp, nop))


if __name__ == "__main__":
    main()
