"""Per-kernel instruction diff of the effect kernels between two gfx950 device objects of effect_kernels.hip -- the check that the
instantiations rtdd_simulate_defocus / _desaturation / _haze launch are unchanged by a later edit (e.g. the FOCUS flag of k_defocus /
k_defocus_tile, k_blend's third mode).  Kernels are matched by demangled name without their parameter lists; for the defocus kernels
of the NEW object a trailing `, false>` template argument (FOCUS off) is dropped.  Branch targets and addresses are normalised.

    F=$(make -s -C realtimedepthdiffusion_amd/csrc print-cxxflags)
    hipcc --offload-arch=gfx950 $F --cuda-device-only -save-temps=obj -o OLD/effect.co -c effect_kernels.hip   # at the parent commit
    hipcc --offload-arch=gfx950 $F --cuda-device-only -save-temps=obj -o NEW/effect.co -c effect_kernels.hip   # at this one
    python scripts/effect_isa_diff.py OLD/effect_kernels-hip-amdgcn-amd-amdhsa-gfx950.out NEW/effect_kernels-hip-amdgcn-amd-amdhsa-gfx950.out

Prints nothing but the count on stderr when every old kernel has its new counterpart with the same instructions; exit status 1 otherwise."""
import difflib
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
PICK = re.compile(r"k_defocus|k_blend|k_sat")


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


def key(name, newer):
    name = name.split("(")[0]
    if newer and "k_defocus" in name:
        name = name.replace(", false>", ">")
    return name


def main(old_path, new_path):
    old = {key(n, False): v for n, v in kernels(old_path).items() if PICK.search(n)}
    new = {key(n, True): v for n, v in kernels(new_path).items() if PICK.search(n)}
    bad = 0
    for n in sorted(old):
        if n not in new:
            print("missing in the new object:", n); bad += 1
        elif old[n] != new[n]:
            print("differs:", n); bad += 1
            for line in list(difflib.unified_diff(old[n], new[n], lineterm=""))[:40]:
                print("  ", line)
    print(f"compared {len(old)} kernels, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
