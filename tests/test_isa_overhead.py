"""CPU: the rollout kernel's substep loop keeps its register-to-register copies and s_nop down.

scripts/isa_overhead.py compiles wk_env_pair.hip to gfx950 assembly with the Makefile's flags and
counts, in the headline kernel's substep loop, the v_mov_b32 / v_mov_b64 from a VGPR and the
s_nop.  The parent of the copy cuts had 393 + 175 = 568 of them in 7,179 instructions
(profiles/copy_cuts_ab.txt); a change that brings the coefficient copies of the rotation's
Horner chains or the assembly copies of the contact-face records back fails here, before any
GPU run.  The kernel must also stay free of scratch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# measured 2026-10-19 on the commit that made the cuts (ROCm 7.2 hipcc): 30 copies (all in the
# C library's large-angle sincos, which no substep rotation takes) + 238 s_nop
RECORDED_COPIES_PLUS_NOPS = 268
SLACK = 1.05  # compiler noise only


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_headline_substep_loop_copies_and_nops():
    import isa_overhead
    text = open(isa_overhead.build_asm(jobs=1)).read()
    res = isa_overhead.loop_stats(text, isa_overhead.HEADLINE)
    assert list(res) == [isa_overhead.HEADLINE], sorted(res)
    c = res[isa_overhead.HEADLINE]
    print(c["total"], "instructions,", c["valu"], "VALU,", c["copies"], "copies,", c["nops"], "s_nop")
    assert c["valu"] > 5000 and c["total"] > c["valu"], c  # (the loop was found: thousands of VALU)
    assert c["copies"] + c["nops"] <= int(RECORDED_COPIES_PLUS_NOPS * SLACK), (c["copies"], c["nops"])
    assert c["scratch"] == 0, c["scratch"]
