"""The scaled sweep pair of the 1080p tile without the instructions that bought nothing (csrc/sweep_tile_sweeps.inc, SCALED && kFromStart).
Counted on the disassembly of the built object (scripts/isa_count.py scaled_pair), without a GPU, in k_sweep_blocked<32, 1024, 3, *, true>.

The pair had 329 VALU instructions with contraction (463 without), 15 of them outside what the reference prescribes: 6 `v_add_f32 v, 0, v`
(the `0 +` in front of pixel 0's left term; without contraction all 24 pixels had one), 4 v_mov_b32 in front of the v_fmac_f32 that
one row's fma(gamma, r - x, x) became, 2 v_mov_b32 of gamma from its SGPR, 2 of omega from its SGPR, and the v_mov_b32 of the publish
counter.  Kept: the `0 +` dropped (-6, -24), gamma in one register for the launch (-2, -2), the sixth row's fma as one v_fma_f32 (-4, with
contraction only).  Not built: omega through LDS (EXPERIMENTS.md), so its 2 movs stay next to the publish counter's.

  * no v_add_f32 with the constant 0;
  * at most 9 - 6 = 3 v_mov_b32;
  * still 24 multiplications by the literal 2^64 and 24 v_med3_f32, and no scratch access;
  * 329 - 12 = 317 VALU instructions with contraction, 463 - 26 = 437 without."""
import os
import re
import sys

import pytest

import realtimedepthdiffusion_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "k_sweep_blockedILi32ELi1024ELi3ELb%dELb1"
VALU = {1: 329 - 6 - 2 - 4, 0: 463 - 24 - 2}
MOVS = 9 - 2 - 4


@pytest.fixture(scope="module")
def isa_count():
    rt.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_count
    return isa_count


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
@pytest.mark.parametrize("contract", [1, 0])
def test_the_lean_scaled_pair_of_the_1080p_tile(isa_count, contract):
    c = isa_count.scaled_pair(kernel=KERNEL % contract)
    by, text = c["by_mnemonic"], c["text"]
    movs = sum(n for k, n in by.items() if k.startswith("v_mov_b32"))
    zero_adds = [t for t in text if re.match(r"v_add_f32\S*\s+v\d+, (0|v\d+), (0|v\d+)$", t) and re.search(r", 0(,|$)", t)]
    print(f"contract {contract}: scaled pair {c['valu']} VALU, {movs} v_mov_b32, {len(zero_adds)} additions of the constant 0; "
          f"{ {k: v for k, v in by.items() if k.startswith('v_')} }")
    assert not zero_adds, zero_adds
    assert not any(t.startswith("v_add_f32") and re.search(r",\s*0(x0+)?\s*(,|$)", t) for t in text)          # (however the operand is spelt)
    assert movs <= MOVS, (movs, by)
    assert c["scale_literals"] == 24, c["scale_literals"]
    assert by.get("v_med3_f32") == 24, by
    assert c["scratch"] == 0 and not any(t.startswith("scratch_") for t in text)
    assert c["valu"] == VALU[contract], (c["valu"], VALU[contract], by)
