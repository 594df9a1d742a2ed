"""No register copy of the sweep kernels may be made under a narrowed EXEC and then be read by every lane.

What this guards (EXPERIMENTS.md "Tile 3"): in k_sweep_blocked<32, 1024, 4, true, true> the register allocator once split the live range
of the lane's column index `lx` inside the short-circuit region of the exchange record's `colok && ...` --

    s_and_saveexec_b64 s[86:87], s[80:81]        ; EXEC &= colok
    ...
    v_mov_b32_e32 v36, v118                      ; lx moves to v36 -- in the lanes of colok only
    s_or_b64 exec, exec, s[86:87]
    ...
    v_mov_b32_e32 v41, v36                       ; every lane takes lx from here on: LDS addresses of the edge rows, lx == 0, lx == LX - 1

-- so the lanes right of the image (the last tile column) went on with a stale v36, published their edge rows into lane 0's LDS slots
and wiped the halo lane's rows at every sweep: errors of up to 2e2 along the last tile column's left border, in that one instantiation.
The compiler is free to do this again wherever a per-lane branch survives in these kernels, so the built objects are checked.

The property, on the disassembly of every k_sweep_blocked, k_sweep_col and k_rbgs_blocked instantiation: inside a straight-line region
that the compiler runs under a narrowed EXEC (s_and_saveexec_b64 <save>, <mask> ... s_or_b64 exec, exec, <save>), a VGPR-to-VGPR
v_mov_b32 of a value that comes from OUTSIDE the region (its source is not written inside it: a masked load or a constant made for the
lanes of the branch is the branch's own business) and whose destination is read behind the region before it is written again must be
the conditional half of a select, that is, its destination was written under the wider EXEC in the straight-line code just in front
of the region (the compiler materialises the other lanes' value there).  A value from outside that changes its register under the
narrowed EXEC and is then read from the new register is the defect: one hit in the object that failed, none in the one before it.
Runs without a GPU."""
import os
import re
import sys

import pytest

import realtimedepthdiffusion_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ("k_sweep_blocked", "k_sweep_col", "k_rbgs_blocked")
HAND_MASKED = ("v_fmac_f32_e32", "v_add_f32_e32")       # what follows a hand-written s_and_saveexec (sweep_common.hpp masked_fmac4 / masked_add4)
IN_FRONT = 48                                           # how far in front of a region the select's other half is looked for
BEHIND = 4000                                           # how far behind it a read is looked for


def _vgprs(text):
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out |= set(range(int(a), int(b) + 1))
    return out | {int(n) for n in re.findall(r"\bv(\d+)\b", text)}


def _split(ins):
    """(mnemonic, VGPRs written, VGPRs read) -- the first operand is the destination except for stores, compares into SGPRs and the like."""
    op, _, rest = ins.partition(" ")
    ops = [o.strip() for o in rest.split(",")] if rest else []
    no_dst = op.startswith(("s_", "ds_write", "ds_bpermute", "global_store", "scratch_store", "buffer_store", "flat_store", "v_cmp", "v_readlane", "v_readfirstlane", "global_atomic"))
    if op.startswith("ds_bpermute"):
        return op, _vgprs(ops[0]), _vgprs(",".join(ops[1:]))
    if no_dst or not ops:
        return op, set(), _vgprs(rest)
    reads = _vgprs(",".join(ops[1:]))
    if op.startswith(("v_fmac", "v_mac", "v_writelane", "v_mov_b32_dpp", "v_cndmask_b32_dpp")) or "dpp" in ins or "sdwa" in ins:
        reads |= _vgprs(ops[0])                         # read-modify-write destinations
    return op, _vgprs(ops[0]), reads


def violations(funcs):
    """[(function, copy, first reader)] over the kernels of KERNELS."""
    bad = []
    for name, instrs in funcs.items():
        if not any(k in name for k in KERNELS):
            continue
        text = [t for _, t, _ in instrs]
        targets = {t for _, _, t in instrs if t is not None}
        addr = [a for a, _, _ in instrs]
        for i, ins in enumerate(text):
            m = re.match(r"s_and_saveexec_b64 (s\[\d+:\d+\]), ", ins)
            if not m or (i + 1 < len(text) and text[i + 1].startswith(HAND_MASKED)):
                continue
            close = f"s_or_b64 exec, exec, {m.group(1)}"
            j = i + 1
            if j < len(text) and text[j].startswith("s_cbranch_execz"):
                j += 1                                  # the skip over the region: it lands on the region's end
            start = j
            while j < len(text) and text[j] != close and not text[j].startswith(("s_cbranch", "s_branch", "s_endpgm", "s_and_saveexec", "s_barrier")) and addr[j] not in targets:
                j += 1
            if j >= len(text) or text[j] != close:
                continue                                # not a straight-line region: nested control flow is the structurizer's, not a copy's, business
            for k in range(start, j):
                c = re.match(r"v_mov_b32_e32 v(\d+), v(\d+)$", text[k])
                if not c:
                    continue
                dst, src = int(c.group(1)), int(c.group(2))
                # a value made inside the region (a masked load, a constant for the lanes of the branch) is the branch's own business:
                # what is looked for is a value from OUTSIDE that changes its register here
                if any(src in _split(text[b])[1] for b in range(start, k)):
                    continue
                # the other half of a select: the destination written in the straight-line code in front of the region
                front = False
                for b in range(i - 1, max(i - 1 - IN_FRONT, -1), -1):
                    if text[b].startswith(("s_cbranch", "s_branch")):
                        break
                    if dst in _split(text[b])[1]:
                        front = True
                        break
                if front:
                    continue
                # ... else nobody may read it behind the region before it is written again (fall-through order)
                for r in range(j + 1, min(j + 1 + BEHIND, len(text))):
                    _, wr, rd = _split(text[r])
                    if dst in rd:
                        bad.append((name, f"{text[k]} (under '{ins}')", text[r]))
                        break
                    if dst in wr:
                        break
    return bad


def _funcs(obj):
    import isa_count
    return isa_count.disassemble(obj)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
@pytest.mark.parametrize("obj", ["sweep_blocked.o", "rbgs_blocked.o"])
def test_no_copy_under_a_narrowed_exec_is_read_by_every_lane(obj):
    rt.build()
    funcs = _funcs(os.path.join(CSRC, obj))
    assert sum(any(k in n for k in KERNELS) for n in funcs) >= (50 if obj.startswith("sweep") else 8), "were the kernels renamed?"
    bad = violations(funcs)
    assert not bad, "\n".join(f"{n}: '{c}' is read by '{r}'" for n, c, r in bad[:10])


def test_the_check_catches_the_copy_it_was_written_for():
    """The defect's own shape, and the select that must not be mistaken for it."""
    head = [(0, "v_mov_b32_e32 v36, 0", None), (4, "global_load_dwordx4 v[34:37], v[4:5], off", None)] + [(8 + 4 * n, "v_add_f32_e32 v60, v61, v62", None) for n in range(60)]
    a = 8 + 4 * 60
    defect = head + [(a, "s_and_saveexec_b64 s[86:87], s[80:81]", None), (a + 4, "v_cmp_le_i32_e64 s[52:53], s63, v107", None),
                     (a + 8, "v_mov_b32_e32 v36, v118", None), (a + 12, "s_or_b64 exec, exec, s[86:87]", None),
                     (a + 16, "v_rcp_f32_e32 v118, v103", None), (a + 20, "v_mov_b32_e32 v41, v36", None), (a + 24, "s_endpgm", None)]
    got = violations({"k_sweep_blocked_fake": defect})
    assert len(got) == 1 and got[0][1].startswith("v_mov_b32_e32 v36, v118") and got[0][2] == "v_mov_b32_e32 v41, v36", got
    select = [(0, "v_mov_b32_e32 v6, 0", None), (4, "s_and_saveexec_b64 s[6:7], s[28:29]", None), (8, "s_cbranch_execz 5", 24),
              (12, "global_load_dwordx4 v[22:25], v[4:5], off", None), (16, "s_waitcnt vmcnt(0)", None), (20, "v_mov_b32_e32 v6, v22", None),
              (24, "s_or_b64 exec, exec, s[6:7]", None), (28, "v_add_f32_e32 v7, v6, v6", None), (32, "s_endpgm", None)]
    assert violations({"k_sweep_blocked_fake": select}) == []
    dead = defect[:-2] + [(a + 20, "v_mov_b32_e32 v36, v1", None), (a + 24, "s_endpgm", None)]          # overwritten before anyone reads it
    assert violations({"k_sweep_blocked_fake": dead}) == []


# ---- the second defect found on the way: an SGPR restored by the VALU right in front of a hand-written VMEM instruction ----------------
def _sgprs(text):
    out = set()
    for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", text):
        out |= set(range(int(a), int(b) + 1))
    return out | {int(n) for n in re.findall(r"\bs(\d+)\b", text)}


def _valu_sgpr_writes(ins):
    """SGPRs a VALU instruction writes: v_readlane / v_readfirstlane / a VOP3 compare (operand 0), a carry-out or v_mad_u64 / v_div_scale (operand 1)."""
    op, _, rest = ins.partition(" ")
    if not op.startswith("v_"):
        return set()
    ops = [o.strip() for o in rest.split(",")]
    out = _sgprs(ops[0]) if ops and ops[0].startswith("s") else set()
    if len(ops) > 1 and ("_co_" in op or op.startswith(("v_mad_u64", "v_mad_i64", "v_div_scale"))) and ops[1].startswith("s"):
        out |= _sgprs(ops[1])
    return out


def vmem_wait_state_violations(funcs, need=5):
    """[(function, VALU writer, VMEM reader, wait states between)]: gfx9 wants `need` wait states between a VALU write of an SGPR and a
    VMEM instruction that reads it (scalar base or offset); the compiler pads its own, nothing inside an asm statement."""
    bad = []
    for name, instrs in funcs.items():
        if not any(k in name for k in KERNELS):
            continue
        text = [t for _, t, _ in instrs]
        for i, ins in enumerate(text):
            if not ins.startswith(("global_", "scratch_", "buffer_", "flat_")):
                continue
            want = _sgprs(ins)
            if not want:
                continue
            states = 0
            for b in range(i - 1, max(i - 1 - need, -1), -1):
                if states >= need:
                    break
                if want & _valu_sgpr_writes(text[b]):
                    bad.append((name, text[b], ins, states))
                    break
                states += 1 + (int(text[b].split()[1], 0) if text[b].startswith("s_nop") else 0)
    return bad


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")
@pytest.mark.parametrize("obj", ["sweep_blocked.o", "rbgs_blocked.o"])
def test_no_vmem_instruction_reads_an_sgpr_the_valu_has_just_written(obj):
    """k_sweep_blocked<32, 512, 6, true, true> once restored the flag words' base with two v_readlane_b32 directly in front of the poll's
    hand-written global_load_dword and read it from a stale pair: an illegal memory access.  Every hand-written statement that addresses
    through a scalar base now opens with the wait states itself (persist_sync.hpp load_flag_at, sweep_common.hpp)."""
    rt.build()
    bad = vmem_wait_state_violations(_funcs(os.path.join(CSRC, obj)))
    assert not bad, "\n".join(f"{n}: '{w}' {s} wait state(s) before '{r}'" for n, w, r, s in bad[:10])


def test_the_wait_state_check_catches_the_restore_it_was_written_for():
    f = {"k_sweep_blocked_fake": [(0, "v_readlane_b32 s66, v221, 8", None), (4, "v_readlane_b32 s67, v221, 9", None),
                                  (8, "global_load_dword v29, v28, s[66:67] sc1", None), (12, "s_endpgm", None)]}
    got = vmem_wait_state_violations(f)
    assert len(got) == 1 and got[0][3] == 0, got
    f["k_sweep_blocked_fake"].insert(2, (6, "s_nop 4", None))
    assert vmem_wait_state_violations(f) == []
    f["k_sweep_blocked_fake"][2] = (6, "s_nop 2", None)
    assert len(vmem_wait_state_violations(f)) == 1
