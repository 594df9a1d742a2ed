"""Per-kernel instruction diff between two gfx950 device objects of one csrc/*.hip file -- the check that an edit left every kernel of
that file instruction for instruction as it was (a host-side refactor; a new template flag that must not touch the old instantiations).
Every function of both objects is compared, matched by its demangled name on both sides alike.  Branch targets and addresses are
normalised: raw code-object bundles differ between two compiles of the same source, the disassembly does not.

    cd realtimedepthdiffusion_amd/csrc                 # the flags hold -I.
    F=$(make -s print-cxxflags)
    hipcc --offload-arch=gfx950 $F --cuda-device-only -c X.hip -o OUT/X.co                # at the parent commit into OLD, here into NEW
    clang-offload-bundler --unbundle --type=o --input=OUT/X.co --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=OUT/X.dev.o
    python scripts/effect_isa_diff.py OLD/X.dev.o NEW/X.dev.o                              # from the repository root

(clang-offload-bundler is /opt/rocm/lib/llvm/bin's.)  Prints "compared N kernels, M differ" on stderr, and for every kernel that differs
or exists in one object only a line and the start of its instruction diff; exit status 1 unless M is 0.

    python scripts/effect_isa_diff.py --multiset OLD/X.dev.o NEW/X.dev.o

is the check for an edit that moves device code into shared helpers: inlining the same statements from another place may rename registers
and reorder independent instructions, which the exact comparison reports and which costs nothing.  Per kernel it compares the MULTISET of
mnemonics (operands dropped: how many of each instruction, in any order) and the kernel's resources from the code object's metadata --
VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes.  A kernel that differs prints the mnemonics whose counts changed and the resources that did."""
import collections
import difflib
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def kernels(path, demangle=True):
    out = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr"] + ["-C"] * demangle + [path], text=True)
    ks, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
        if m:
            cur = m.group(1); ks[cur] = []; continue
        if cur and line.strip() and not line.startswith("Disassembly"):
            ins = re.sub(r"//.*", "", line).strip()
            ins = re.sub(r"<[^>]*>", "<L>", ins)
            if ins and ins != "...":
                ks[cur].append(ins)
    return ks


RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def resources(path):
    """demangled kernel name -> its RESOURCES, from the amdhsa.kernels list of the metadata note"""
    out = subprocess.check_output([READELF, "--notes", path], text=True)
    recs = []
    for line in out.splitlines():
        m = re.match(r"^  (- |  )(\.\w+):\s*(\S*)$", line)
        if m and m.group(1) == "- ":
            recs.append({})
        if m and recs:
            recs[-1][m.group(2)] = m.group(3)
    demangled = dict(zip(kernels(path, demangle=False), kernels(path)))             # (the same functions in the same order)
    return {demangled[r[".name"]]: tuple(int(r[k]) for k in RESOURCES) for r in recs}


def main_multiset(old_path, new_path):
    old, new, rold, rnew = kernels(old_path), kernels(new_path), resources(old_path), resources(new_path)
    names = sorted(n for n in old.keys() | new.keys() if n in rold or n in rnew)       # kernels only: they alone have resources
    bad = 0
    for n in names:
        if n not in new or n not in old:
            print("missing in the", "new" if n not in new else "old", "object:", n); bad += 1; continue
        a, b = (collections.Counter(i.split()[0] for i in k[n]) for k in (old, new))
        if a == b and rold[n] == rnew[n]:
            continue
        print("differs:", n); bad += 1
        for m in sorted(a.keys() | b.keys()):
            if a[m] != b[m]:
                print(f"   {m}: {a[m]} -> {b[m]}")
        for k, x, y in zip(RESOURCES, rold[n], rnew[n]):
            if x != y:
                print(f"   {k}: {x} -> {y}")
    print(f"compared {len(names)} kernels by mnemonic multiset and resources, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    bad = 0
    for n in sorted(old.keys() | new.keys()):
        if n not in new:
            print("missing in the new object:", n); bad += 1
        elif n not in old:
            print("missing in the old object:", n); bad += 1
        elif old[n] != new[n]:
            print("differs:", n); bad += 1
            for line in list(difflib.unified_diff(old[n], new[n], lineterm=""))[:40]:
                print("  ", line)
    print(f"compared {len(old.keys() | new.keys())} kernels, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main_multiset(*sys.argv[2:4]) if sys.argv[1] == "--multiset" else main(sys.argv[1], sys.argv[2]))
