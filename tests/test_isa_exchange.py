"""The persistent sweep's halo exchange works from a per-thread record built once per launch (csrc/sweep_blocked.hip `xrec`): no
coordinate, address or predicate is recomputed between the sweeps of two blocks.  Checked on the disassembly of the built object
(scripts/isa_count.py exchange_region), without a GPU, in EVERY persistent instantiation of k_sweep_blocked:
  * nothing on any path from the sweep-pair loop's exit back to its head -- the exchange, the polling loop, the time-out reports, the
    full-divide variant's sweeps, the block loop's back edge -- is a 64-bit multiply or shift-add (v_mad_u64_u32, v_mad_i64_i32,
    v_lshl_add_u64, v_lshlrev_b64: per-lane 64-bit address arithmetic);
  * on the path of a wave that meets no group straddling the image's right edge, nothing behind the halo loads' wait is a v_cndmask or a
    v_mov that names a tile register: the loads' destinations ARE the tile's registers, and the select is taken only by the waves that need it."""
import os
import sys

import pytest

import realtimedepthdiffusion_amd as rt
import tile_geometry as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def listing():
    rt.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_count
    funcs = isa_count.disassemble(os.path.join(CSRC, "sweep_blocked.o"))
    kernels = isa_count.persistent_kernels(funcs)
    assert len(kernels) == 26, sorted(kernels)
    return isa_count, {n: (funcs[n], isa_count.exchange_region(funcs[n], g)) for n, g in kernels.items()}


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
def test_no_64_bit_address_arithmetic_between_the_sweeps_of_two_blocks(listing):
    isa_count, kernels = listing
    for name, (instrs, r) in kernels.items():
        assert len(r["region"]) > 100 and sum(instrs[u][1].startswith("s_barrier") for u in r["region"]) >= 2, f"{name}: the region holds no exchange"
        wide = [instrs[u][1] for u in r["region"] if instrs[u][1].startswith(isa_count.WIDE_ADDRESS_OPS)]
        assert not wide, f"{name}: {len(wide)} 64-bit multiplies / shift-adds between the sweeps of two blocks, first '{wide[0]}'"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
@pytest.mark.parametrize("contract", [1, 0])
@pytest.mark.parametrize("tile", tg.ROW_TILES)
def test_nothing_moves_or_selects_a_tile_register_behind_the_halo_loads_wait(listing, tile, contract):
    """One case per instantiation.  (What it took beyond the record itself, csrc/sweep_blocked.hip and sweep_tile_sweeps.inc: the two divide
    variants of a block as consecutive loops -- as an if / else every block moved the whole tile twice; the full-divide variant's odd
    tail sweep inside its pair loop -- behind it the two-row tiles moved x_{k-1} at every block; and, in the one-row tiles, the row a
    sweep has written passed through one empty statement as four consecutive registers.)"""
    isa_count, kernels = listing
    LX, NT, g = tg.TILES[tile]
    name = next(n for n in kernels if f"k_sweep_blockedILi{LX}ELi{NT}ELi{g}ELb{contract}ELb1EEE" in n)
    instrs, r = kernels[name]
    path = [instrs[u][1] for u in r["path"]]
    assert sum(t.startswith("global_store_dwordx4") for t in path) == 2 * g and sum(t.startswith("global_load_dwordx4") for t in path) == 2 * g, \
        f"{name}: the path does not store and load {g} rows of two planes"
    assert len(r["tile"]) == 8 * g and r["behind"], name
    for u in r["behind"]:
        t = instrs[u][1]
        assert not t.startswith("v_cndmask"), f"{name}: '{t}' behind the halo loads' wait on the path without the straddle select"
        assert not (t.startswith("v_mov") and isa_count._vgprs(t) & r["tile"]), f"{name}: '{t}' moves a tile register behind the halo loads' wait"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
def test_the_census_of_the_1080p_exchange(listing):
    """scripts/isa_count.py exchange_census(): what EXPERIMENTS.md quotes.  The path of the 1080p instantiation holds its two barriers,
    one record read and no address arithmetic wider than an add per row."""
    isa_count, _ = listing
    c = isa_count.exchange_census()
    by = c["by_mnemonic"]
    assert c["wide_address_ops"] == 0 and c["v_cndmask"] == 0 and by.get("s_barrier") == 2, c
    assert by.get("ds_read_b96", 0) + by.get("ds_read_b128", 0) == 1 and by.get("global_store_dwordx4") == 6 and by.get("global_load_dwordx4") == 6, by
