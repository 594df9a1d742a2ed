"""Nothing waits on memory between a halo exchange's first barrier and the store of the tile's flag (csrc/persist_sync.hpp
exchange_wait_at): that stretch is where every tile of the grid waits for its neighbours' flags, and the tile whose flag the testing aid
RTDD_OPT_DEBUG_WITHHOLD_TILE withholds is a kernel argument, compared in scalar registers -- not a word of sync_words read back at every
one of a solve's 124 exchanges.  Checked on the disassembly of the built objects, without a GPU, in EVERY persistent instantiation of
k_sweep_blocked (26) and k_rbgs_blocked (8).

How the stretch is found (control flow as scripts/isa_count.py _successors() sees it): the strip stores are the 16-byte sc1 stores (of a
sweep kernel: those inside isa_count.exchange_region()); the exchange's first barrier is the first s_barrier behind one of them; the
flag store is the NEAREST 4-byte sc1 store behind that barrier (the status word's store lies behind the polling loop); the stretch is
every instruction on some barrier-free path from the one to the other."""
import os
import re
import sys

import pytest

import realtimedepthdiffusion_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="ROCm LLVM tools not present")


@pytest.fixture(scope="module")
def isa_count():
    rt.build()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_count
    return isa_count


def _is_sc1(txt, mnemonic):
    return txt.split()[0] == mnemonic and txt.rstrip().endswith("sc1")


def _bfs(instrs, index, isa_count, starts, stop, backward_of=None):
    """Indices reachable from `starts` (exclusive of them unless reached again) without passing THROUGH an instruction `stop` accepts;
    the stopping instructions themselves are returned with their distance.  backward_of: a predecessor map to walk instead."""
    dist, todo = {}, [(s, 0) for s in starts]
    seen = set(starts)
    while todo:
        nxt = []
        for u, d in todo:
            for v in (backward_of.get(u, ()) if backward_of is not None else isa_count._successors(instrs, index, u)):
                if v in seen:
                    continue
                seen.add(v); dist[v] = d + 1
                if not stop(instrs[v][1]):
                    nxt.append((v, d + 1))
        todo = nxt
    return dist


def stretches(instrs, isa_count, strip_stores):
    """[(barrier index, flag store index, [indices strictly between them on some barrier-free path])] of one kernel."""
    index = {a: i for i, (a, _, _) in enumerate(instrs)}
    preds = {}
    for u in range(len(instrs)):
        for v in isa_count._successors(instrs, index, u):
            preds.setdefault(v, []).append(u)
    is_barrier = lambda t: t.startswith("s_barrier")
    first = _bfs(instrs, index, isa_count, strip_stores, is_barrier)
    barriers = sorted(u for u in first if is_barrier(instrs[u][1]))
    out = []
    for b in barriers:
        fwd = _bfs(instrs, index, isa_count, [b], lambda t: is_barrier(t) or _is_sc1(t, "global_store_dword"))
        flags = [u for u in fwd if _is_sc1(instrs[u][1], "global_store_dword")]
        assert flags, f"no 4-byte sc1 store behind the barrier at {instrs[b][0]:#x}"
        f = min(flags, key=lambda u: fwd[u])
        bwd = _bfs(instrs, index, isa_count, [f], is_barrier, backward_of=preds)
        assert b in bwd, "the flag store is not reached from the exchange's first barrier"
        out.append((b, f, sorted(u for u in fwd if u in bwd and u not in (b, f) and not is_barrier(instrs[u][1]))))
    return out


def check(name, instrs, isa_count, strip_stores):
    assert strip_stores, f"{name}: no 16-byte sc1 strip store"
    found = stretches(instrs, isa_count, strip_stores)
    assert found, f"{name}: no barrier behind the strip stores"
    for b, f, between in found:
        assert len(between) <= 40, f"{name}: {len(between)} instructions between the barrier and the flag store: not the stretch this test means"
        for u in between:
            t = instrs[u][1]
            assert not t.startswith(("global_load", "s_load", "s_buffer_load", "buffer_load", "flat_load", "scratch_load")), \
                f"{name}: '{t}' between the exchange's first barrier and the flag store '{instrs[f][1]}'"
            assert not (t.startswith("s_waitcnt") and "vmcnt" in t), f"{name}: '{t}' between the exchange's first barrier and the flag store"


def test_sweep_kernels_flag_store_waits_for_no_load(isa_count):
    funcs = isa_count.disassemble(os.path.join(CSRC, "sweep_blocked.o"))
    kernels = isa_count.persistent_kernels(funcs)
    assert len(kernels) == 26, sorted(kernels)
    for name, g in kernels.items():
        instrs = funcs[name]
        region = isa_count.exchange_region(instrs, g)["region"]
        check(name, instrs, isa_count, [u for u in region if _is_sc1(instrs[u][1], "global_store_dwordx4")])


def test_red_black_kernels_flag_store_waits_for_no_load(isa_count):
    funcs = isa_count.disassemble(os.path.join(CSRC, "rbgs_blocked.o"))
    kernels = [n for n in funcs if re.search(r"k_rbgs_blockedILi\d+ELi\d+ELi\d+ELb[01]ELb[01]ELb1EEE", n)]
    assert len(kernels) == 8, sorted(kernels)           # two tiles x FP contraction x SOR
    for name in kernels:
        instrs = funcs[name]
        check(name, instrs, isa_count, [u for u, (_, t, _) in enumerate(instrs) if _is_sc1(t, "global_store_dwordx4")])
