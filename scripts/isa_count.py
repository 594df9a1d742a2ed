#!/usr/bin/env python3
"""Static VALU instruction count of the Jacobi sweep's hot loop, from the disassembly of the BUILT object.

bench.py prices the sweep's VALU roofline with "VALU operations per pixel-sweep" -- a count of the instructions the fast path of
k_sweep_blocked<32, 1024, 3, true, true> issues for one pair of sweeps over a thread's 12 pixels.  That number used to be a constant
typed into bench.py; this module recounts it from realtimedepthdiffusion_amd/csrc/sweep_blocked.o so that the constant cannot drift
away from the code (tests/test_isa_hazards.py asserts the two agree; scripts/make_counters_json.py refuses to write a record otherwise).

How the loop is found: every backward branch of the function closes a loop; from its target the instructions are walked along the
FALL-THROUGH path (conditional branches not taken -- the waiting loops, the full-divide path and the time-out reports all hang off
taken branches, by construction: __builtin_expect -- unconditional branches followed) until the walk reaches a branch back to the loop's
head.  The sweep pair is the loop whose fall-through path holds exactly 24 v_med3_f32 (12 pixels x 2 sweeps) and no v_div_scale_f32.
A persistent instantiation has a second such loop, the sweep pair of a wave in scaled mode (csrc/sweep_common.hpp: div_scaled4 in the from-start tile, the 1080p one, div_scaled in the others): it is told
apart by its multiplications by the literal 2^64 and is not the loop sweep_pair() counts -- it belongs to the exchange's `region`, like the
full-divide variant's loops.  scaled_pair() is its census: in the tile that enters the mode at sweep 0 (the 1080p tile) it is the loop the
waves actually run; in every other persistent tile it finds the seven-operation loop of the on-demand mode.  kernel_resources() reads VGPRs and private segment sizes of the persistent instantiations from the code object's notes.
"""
import glob
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HOT_KERNEL = "k_sweep_blockedILi32ELi1024ELi3ELb1ELb1"         # k_sweep_blocked<32, 1024, 3, true, true>: the 1080p persistent instantiation
PIXELS_PER_THREAD = 12


def disassemble(obj):
    """{mangled function name: [(address, instruction text, branch target address or None), ...]} of the gfx950 code object inside `obj`."""
    tmp = tempfile.mkdtemp(prefix="isa_count_")
    try:
        local = os.path.join(tmp, "x.o")
        shutil.copy(obj, local)
        subprocess.check_call([OBJDUMP, "--offloading", local], stdout=subprocess.DEVNULL, cwd=tmp)
        dev = sorted(glob.glob(local + ".*gfx950*"))
        if not dev:
            raise RuntimeError("no gfx950 code object in " + obj)
        text = "\n".join(subprocess.check_output([OBJDUMP, "-d", d], text=True) for d in dev)      # (a shared library holds one code object per translation unit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    funcs, cur, base = {}, None, 0
    for line in text.split("\n"):
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:", line)
        if m:
            base = int(m.group(1), 16); cur = funcs.setdefault(m.group(2), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):\s+[0-9A-Fa-f ]+(?:<[^>+]+\+0x([0-9a-fA-F]+)>)?\s*$", line)
        if m and cur is not None:
            cur.append((int(m.group(2), 16), m.group(1).strip(), base + int(m.group(3), 16) if m.group(3) else None))
    return funcs


SCALE_LITERAL = "0x5f800000"                  # bits(2^64): only the scaled divides multiply by it (div_scaled4 in the from-start tile, div_scaled in the on-demand tiles, div_tiny)


def is_fast_pair(path, pixels):
    """The fall-through path of the FAST sweep pair of a thread of `pixels` pixels: one clamp per pixel and sweep, no full divide, no scaled divide."""
    return sum(t.startswith("v_med3_f32") for t in path) == 2 * pixels and not any(t.startswith("v_div_scale") or SCALE_LITERAL in t for t in path)


def fallthrough_loops(instrs):
    """For every backward branch: the instructions on the fall-through path from its target back to a branch to that target."""
    index = {a: i for i, (a, _, _) in enumerate(instrs)}
    heads = sorted({t for a, txt, t in instrs if t is not None and t <= a and txt.startswith(("s_cbranch", "s_branch")) and t in index})
    loops = []
    for head in heads:
        i, path, steps = index[head], [], 0
        while 0 <= i < len(instrs) and steps < 20000:
            a, txt, t = instrs[i]
            steps += 1
            if txt.startswith(("s_cbranch", "s_branch")) and t == head:
                loops.append((head, path))
                break
            if txt.startswith("s_endpgm"):
                break
            path.append(txt)
            if txt.startswith("s_branch") and t is not None:
                if t not in index:
                    break
                i = index[t]
                continue
            i += 1
    return loops


def sweep_pair(obj=None, kernel=HOT_KERNEL):
    """Instruction census of the fast sweep pair: {'valu', 'salu', 'lds', 'per_pixel_sweep', 'by_mnemonic'}."""
    if obj is None:                                # the object where it exists (a build tree), else the library itself (what travels to a GPU box)
        obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "sweep_blocked.o")
        if not os.path.exists(obj):
            obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "librtdd.so")
    funcs = disassemble(obj)
    names = [n for n in funcs if kernel in n]
    if len(names) != 1:
        raise RuntimeError(f"{kernel}: {len(names)} functions match in {obj}")
    found = []
    for head, path in fallthrough_loops(funcs[names[0]]):
        if is_fast_pair(path, PIXELS_PER_THREAD):
            found.append(path)
    if len(found) != 1:
        raise RuntimeError(f"{kernel}: expected ONE loop with 24 v_med3_f32 and no full divide on its fall-through path, found {len(found)}")
    path = found[0]
    by = {}
    for t in path:
        by[t.split()[0]] = by.get(t.split()[0], 0) + 1
    valu = sum(n for k, n in by.items() if k.startswith("v_"))
    return {"valu": valu, "salu": sum(n for k, n in by.items() if k.startswith("s_")), "lds": sum(n for k, n in by.items() if k.startswith("ds_")),
            "instructions": len(path), "per_pixel_sweep": valu / (2.0 * PIXELS_PER_THREAD), "by_mnemonic": dict(sorted(by.items(), key=lambda kv: -kv[1]))}


def is_scaled_pair(path, pixels):
    """The fall-through path of the SCALED sweep pair (a wave in scaled mode, csrc/sweep_common.hpp div_scaled4 / div_scaled): one clamp per pixel and sweep,
    no full divide, and multiplications by the literal 2^64."""
    return sum(t.startswith("v_med3_f32") for t in path) == 2 * pixels and not any(t.startswith("v_div_scale") for t in path) and any(SCALE_LITERAL in t for t in path)


def scaled_pair(obj=None, kernel=HOT_KERNEL, pixels=PIXELS_PER_THREAD):
    """Instruction census of the scaled sweep pair of one persistent instantiation, as sweep_pair() gives it for the fast pair, plus
    'scale_literals' (multiplications by 2^64), 'scratch' (scratch accesses) and 'text' (the instructions themselves)."""
    if obj is None:
        obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "sweep_blocked.o")
        if not os.path.exists(obj):
            obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "librtdd.so")
    funcs = disassemble(obj)
    names = [n for n in funcs if kernel in n]
    if len(names) != 1:
        raise RuntimeError(f"{kernel}: {len(names)} functions match in {obj}")
    found = [path for head, path in fallthrough_loops(funcs[names[0]]) if is_scaled_pair(path, pixels)]
    if len(found) != 1:
        raise RuntimeError(f"{kernel}: expected ONE loop with {2 * pixels} v_med3_f32, no full divide and multiplications by 2^64 on its fall-through path, found {len(found)}")
    path = found[0]
    by = {}
    for t in path:
        by[t.split()[0]] = by.get(t.split()[0], 0) + 1
    valu = sum(n for k, n in by.items() if k.startswith("v_"))
    return {"valu": valu, "salu": sum(n for k, n in by.items() if k.startswith("s_")), "lds": sum(n for k, n in by.items() if k.startswith("ds_")),
            "instructions": len(path), "per_pixel_sweep": valu / (2.0 * pixels), "scale_literals": sum(SCALE_LITERAL in t for t in path),
            "scratch": sum(t.startswith(("scratch_", "buffer_load", "buffer_store")) for t in path),
            "by_mnemonic": dict(sorted(by.items(), key=lambda kv: -kv[1])), "text": path}


def kernel_resources(obj=None):
    """{mangled name: {'vgprs', 'private_segment'}} of the persistent instantiations, from the code object's notes.  (`vgprs` is the
    kernel's whole register count, AGPRs included: 128 or fewer admit the four waves per SIMD that a 1024-thread workgroup needs; LDS is not looked at.)"""
    if obj is None:
        obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "sweep_blocked.o")
        if not os.path.exists(obj):
            obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "librtdd.so")
    tmp = tempfile.mkdtemp(prefix="isa_count_")
    try:
        local = os.path.join(tmp, "x.o")
        shutil.copy(obj, local)
        subprocess.check_call([OBJDUMP, "--offloading", local], stdout=subprocess.DEVNULL, cwd=tmp)
        notes = "\n".join(subprocess.check_output([os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf"), "--notes", d], text=True) for d in sorted(glob.glob(local + ".*gfx950*")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or not re.search(r"k_sweep_blockedILi\d+ELi\d+ELi\d+ELb[01]ELb1EEE", name.group(1)):
            continue
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        out[name.group(1)] = {"vgprs": vgprs, "private_segment": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))}
    return out


# ---- the halo exchange of the persistent instantiations -------------------------------------------------------------------------
WIDE_ADDRESS_OPS = ("v_mad_u64_u32", "v_mad_i64_i32", "v_lshl_add_u64", "v_lshlrev_b64")      # 64-bit multiplies and shift-adds: per-lane address arithmetic


def persistent_kernels(funcs):
    """{mangled name: G} of the persistent instantiations k_sweep_blocked<LX, NT, G, CONTRACT, true>."""
    out = {}
    for n in funcs:
        m = re.search(r"k_sweep_blockedILi(\d+)ELi(\d+)ELi(\d+)ELb[01]ELb1EEE", n)
        if m:
            out[n] = int(m.group(3))
    return out


def _vgprs(text):
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out |= set(range(int(a), int(b) + 1))
    return out | {int(n) for n in re.findall(r"\bv(\d+)\b", text)}


def _is_branch(txt):
    return txt.startswith(("s_cbranch", "s_branch"))


def _successors(instrs, index, i):
    """Where control can go from instruction i.  A forward s_cbranch_execz over a loop-free span that holds a 16-byte sc1 access or a
    v_cndmask is NOT taken: that is how the compiler skips a masked strip store, halo load or select when no lane is active, and the
    census is of a wave in which some lane is (every wave of the 1080p tile stores and loads halo columns).  Every other masked span --
    the flag store of thread 0, the flag poll of eight lanes of wave 0 -- can be skipped."""
    a, txt, t = instrs[i]
    if txt.startswith("s_endpgm"):
        return []
    if txt.startswith("s_branch"):
        return [index[t]] if t in index else []
    if txt.startswith("s_cbranch") and t in index:
        j = index[t]
        if txt.startswith("s_cbranch_execz") and j > i and not any(_is_branch(x) and tt is not None and tt <= aa for aa, x, tt in instrs[i + 1:j]) and \
                any(("dwordx4" in x and x.rstrip().endswith("sc1")) or x.startswith("v_cndmask") for _, x, _ in instrs[i + 1:j]):
            return [i + 1]
        return [i + 1, j]
    return [i + 1] if i + 1 < len(instrs) else []


def exchange_region(instrs, G):
    """Of one persistent instantiation: what lies between the fast sweep-pair loop's exit and its next entry -- the halo exchange, the
    block loop's back edge and the next block's prologue.  Returns
      region   every instruction on SOME path from the loop (its exit, or a branch to one of its out-of-line parts) back into it that does not
               lead through the loop: the exchange, the full-divide variant's loops, the polling and waiting loops, the time-out reports;
               the write-back behind the block loop cannot return to the loop and is not part of it.  By index;
      path     the SHORTEST such path under _successors(): a wave that stores and loads its rows, does not poll, meets no straddling
               group and runs no full-divide sweep;
      behind   the part of `path` behind the s_waitcnt vmcnt(0) that follows the last 16-byte sc1 halo load;
      tile     the VGPRs the halo loads on the path write (the tile's registers)."""
    index = {a: i for i, (a, _, _) in enumerate(instrs)}
    head = None
    for h, path in fallthrough_loops(instrs):
        if is_fast_pair(path, 4 * G):
            if head is not None:
                raise RuntimeError("two sweep-pair loops without a full divide")
            head = index[h]
    if head is None:
        raise RuntimeError("no sweep-pair loop found")
    # the loop's fall-through path (its hot body), and where control can leave it: the loop's exit and the branches to its out-of-line parts
    # (waiting loops, the full-divide redo), which come straight back
    hot, i = set(), head
    while not (_is_branch(instrs[i][1]) and instrs[i][2] == instrs[head][0]):
        hot.add(i)
        i = index[instrs[i][2]] if instrs[i][1].startswith("s_branch") else i + 1
    hot.add(i)
    exits = sorted({v for u in hot for v in ([index[instrs[u][2]]] if _is_branch(instrs[u][1]) and instrs[u][2] in index else []) +
                    ([] if instrs[u][1].startswith(("s_branch", "s_endpgm")) else [u + 1]) if v not in hot})

    def bfs(starts):                               # breadth first under _successors(), never THROUGH the sweep-pair loop: distances and predecessors
        dist, prev, todo = {e: 0 for e in starts}, {}, list(starts)
        while todo:
            nxt = []
            for u in todo:
                if u in hot:
                    continue
                for v in _successors(instrs, index, u):
                    if v not in dist:
                        dist[v] = dist[u] + 1; prev[v] = u; nxt.append(v)
            todo = nxt
        return dist, prev

    def walk_back(prev, u):
        out = [u]
        while out[-1] in prev:
            out.append(prev[out[-1]])
        return out[::-1]
    dist, prev = bfs(exits)
    back = {u for u in dist if u in hot}            # of everything reachable from the exits: what can reach the sweep-pair loop again
    if not back:
        raise RuntimeError("the block loop's back edge was not found")
    changed = True
    while changed:
        changed = False
        for u in dist:
            if u not in back and any(v in back for v in _successors(instrs, index, u)):
                back.add(u); changed = True
    back -= hot
    # the path: exit -> the nearest 16-byte sc1 strip store -> the farthest 16-byte sc1 halo load behind it -> the head
    def is_x4(u, kind):
        return instrs[u][1].startswith(kind + "_dwordx4") and instrs[u][1].rstrip().endswith("sc1")
    stores = [u for u in back if is_x4(u, "global_store")]
    if not stores:
        raise RuntimeError("no 16-byte sc1 strip store between the sweeps of two blocks")
    s0 = min(stores, key=lambda u: dist[u])
    d1, p1 = bfs([s0])
    l1 = max((u for u in d1 if u in back and is_x4(u, "global_load")), key=lambda u: d1[u], default=None)
    if l1 is None:                                 # (the acquire variant has plain loads: no path behind a wait to speak of)
        l1 = s0
    d2, p2 = bfs([l1])
    entry = min((u for u in d2 if u in hot), key=lambda u: d2[u])
    path = walk_back(prev, s0) + walk_back(p1, l1)[1:] + walk_back(p2, entry)[1:-1]
    loads = [k for k, u in enumerate(path) if instrs[u][1].startswith("global_load_dwordx4") and instrs[u][1].rstrip().endswith("sc1")]
    tile, behind = set(), []
    if loads:
        for k in loads:
            tile |= _vgprs(instrs[path[k]][1].split(None, 1)[1].split(",")[0])
        w = next(k for k in range(loads[-1], len(path)) if instrs[path[k]][1].startswith("s_waitcnt") and "vmcnt(0)" in instrs[path[k]][1])
        behind = path[w + 1:]
    return {"region": sorted(back), "path": path, "behind": behind, "tile": tile}


def exchange_census(obj=None, kernel=HOT_KERNEL):
    """Instruction census of the exchange path of one persistent instantiation (default: the 1080p one)."""
    if obj is None:
        obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "sweep_blocked.o")
        if not os.path.exists(obj):
            obj = os.path.join(ROOT, "realtimedepthdiffusion_amd", "librtdd.so")
    funcs = disassemble(obj)
    names = [n for n in persistent_kernels(funcs) if kernel in n]
    if len(names) != 1:
        raise RuntimeError(f"{kernel}: {len(names)} persistent instantiations match in {obj}")
    instrs = funcs[names[0]]
    r = exchange_region(instrs, persistent_kernels(funcs)[names[0]])
    txt = [instrs[u][1] for u in r["path"]]
    by = {}
    for t in txt:
        by[t.split()[0]] = by.get(t.split()[0], 0) + 1
    return {"instructions": len(txt), "valu": sum(n for k, n in by.items() if k.startswith("v_")), "salu": sum(n for k, n in by.items() if k.startswith("s_")),
            "behind_the_wait": len(r["behind"]), "wide_address_ops": sum(n for k, n in by.items() if k.startswith(WIDE_ADDRESS_OPS)),
            "v_mov": sum(n for k, n in by.items() if k.startswith("v_mov")), "v_cndmask": sum(n for k, n in by.items() if k.startswith("v_cndmask")),
            "region_instructions": len(r["region"]), "by_mnemonic": dict(sorted(by.items(), key=lambda kv: -kv[1]))}


if __name__ == "__main__":
    import json
    import sys
    c = sweep_pair(*sys.argv[1:2])
    print(json.dumps(c, indent=1))
    print(json.dumps(exchange_census(*sys.argv[1:2]), indent=1))
    c = scaled_pair(*sys.argv[1:2])
    del c["text"]
    print(json.dumps(c, indent=1))
