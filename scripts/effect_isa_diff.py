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
VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes.  A kernel that differs prints the mnemonics whose counts changed and the resources that did.
Instructions behind a kernel's last s_endpgm are not counted: they are padding up to the next function's alignment and never run.

    python scripts/effect_isa_diff.py [--multiset] --rename 'OLD=NEW' [--rename ...] OLD/X.dev.o NEW/X.dev.o

compares the old object's function OLD with the new object's NEW (demangled names, as the tool prints them): for an edit that renames a
kernel or turns two kernels into instantiations of one template."""
import argparse
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


def renamed(d, renames):
    return {renames.get(k, k): v for k, v in d.items()}


def executed(ins):
    """The instructions up to and including the last s_endpgm (all of them where there is none: a device function)."""
    ends = [i for i, x in enumerate(ins) if x.split()[0] == "s_endpgm"]
    return ins[:ends[-1] + 1] if ends else ins


def main_multiset(old_path, new_path, renames):
    old, new, rold, rnew = renamed(kernels(old_path), renames), kernels(new_path), renamed(resources(old_path), renames), resources(new_path)
    names = sorted(n for n in old.keys() | new.keys() if n in rold or n in rnew)       # kernels only: they alone have resources
    bad = 0
    for n in names:
        if n not in new or n not in old:
            print("missing in the", "new" if n not in new else "old", "object:", n); bad += 1; continue
        a, b = (collections.Counter(i.split()[0] for i in executed(k[n])) for k in (old, new))
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


def main(old_path, new_path, renames):
    old, new = renamed(kernels(old_path), renames), kernels(new_path)
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--multiset", action="store_true", help="compare mnemonic multisets and resources instead of the instruction sequences")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="the old object's function OLD is the new object's NEW (repeatable)")
    ap.add_argument("old"); ap.add_argument("new")
    args = ap.parse_args()
    if any("=" not in r for r in args.rename):
        ap.error("--rename takes OLD=NEW")
    names = dict(r.split("=", 1) for r in args.rename)
    sys.exit((main_multiset if args.multiset else main)(args.old, args.new, names))
