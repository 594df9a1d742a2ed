"""The sweep pair that the waves of the 1080p solve run: scaled mode entered at sweep 0 (csrc/sweep_blocked.hip kFromStart), every quotient by
the four-operation div_scaled4 (csrc/sweep_common.hpp) with the divisors and reciprocals held as d * 2^64 and y * 2^-64.  Counted on the
disassembly of the built object (scripts/isa_count.py scaled_pair), without a GPU, in k_sweep_blocked<32, 1024, 3, *, true>, both
contraction settings:

  * 24 multiplications by the literal 2^64 -- one per pixel and sweep (12 pixels x 2 sweeps); the seven-operation div_scaled had three
    scale multiplications per pixel, 72;
  * 24 v_med3_f32: the loop is a whole sweep pair;
  * no v_lshl_add_u32 and no v_min3_u32 (the tiny test is gone), no v_div_scale_f32 (no IEEE divide), no scratch access;
  * no more VALU instructions than the fast pair of the same instantiation, which stays what tests/test_isa_hazards.py pins.

And the registers: the 1080p instantiations stay within the 128 registers that four waves per SIMD allow, with no private segment."""
import os
import sys

import pytest

import realtimedepthdiffusion_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "k_sweep_blockedILi32ELi1024ELi3ELb%dELb1"


@pytest.fixture(scope="module")
def isa_count():
    rt.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_count
    return isa_count


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
@pytest.mark.parametrize("contract", [1, 0])
def test_the_scaled_pair_of_the_1080p_tile(isa_count, contract):
    fast = isa_count.sweep_pair(kernel=KERNEL % contract)
    c = isa_count.scaled_pair(kernel=KERNEL % contract)
    by, text = c["by_mnemonic"], c["text"]
    print(f"contract {contract}: scaled pair {c['valu']} VALU ({c['per_pixel_sweep']:.2f} per pixel-sweep), fast pair {fast['valu']}; "
          f"{ {k: v for k, v in by.items() if k.startswith('v_')} }")
    assert c["scale_literals"] == 24, c["scale_literals"]
    assert all(t.startswith("v_mul_f32") for t in text if isa_count.SCALE_LITERAL in t)          # 2^64 is a literal OF THE MULTIPLICATION
    assert by.get("v_med3_f32") == 24, by
    for gone in ("v_lshl_add_u32", "v_min3_u32", "v_min_u32", "v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32"):
        assert not any(k.startswith(gone) for k in by), (gone, by)
    assert c["scratch"] == 0 and not any(t.startswith("scratch_") for t in text)
    assert not any(k.startswith("v_cmp_gt_u32") for k in by), by                                        # no compare of a tiny test
    assert c["valu"] <= fast["valu"], (c["valu"], fast["valu"])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
def test_the_1080p_tile_keeps_four_waves_per_simd_and_no_scratch(isa_count):
    res = isa_count.kernel_resources()
    assert len(res) == 26, sorted(res)
    for contract in (1, 0):
        name = next(n for n in res if (KERNEL % contract) in n)
        r = res[name]
        print(name, r)
        assert r["vgprs"] <= 128 and r["private_segment"] == 0, (name, r)          # 128 registers or fewer: four waves per SIMD
