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
or exists in one object only a line and the start of its instruction diff; exit status 1 unless M is 0."""
import difflib
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(path):
    out = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", "-C", path], text=True)
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
    sys.exit(main(sys.argv[1], sys.argv[2]))
