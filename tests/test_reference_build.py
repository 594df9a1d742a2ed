"""The reference's own GPU code as build() leaves it in oracle/_ref/ (oracle/ref.mk), checked without a GPU.

tests/test_gpu_reference.py runs these two libraries next to the product and skips when they are missing; this file is what fails if
build() stopped producing them.  Besides existence, symbols and symbol binding it pins the FP contraction of each build on its ISA: the
GPU tests compare RTDD_OPT_FP_CONTRACT = 0 with libref_c0.so and = 1 with libref_c1.so bit for bit, so a toolchain that fused
differently should fail here, with a message that names the expression, not there as an unexplained bit difference.
Skipped only when the reference tree itself is absent (oracle.reference_dir())."""
import os
import re
import shutil
import subprocess

import pytest

import oracle
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FMA = ("v_fma_f32", "v_fmac_f32", "v_fmamk_f32", "v_fmaak_f32")

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(oracle.reference_dir(), "src", "GPUSolver.cu")),
                                reason=f"no reference tree at {oracle.reference_dir()} (RTDD_REFERENCE_DIR)")


@pytest.fixture(scope="module")
def built():
    assert oracle.build_ref() == ref.REF_DIR, "oracle.build_ref() did not build oracle/_ref/"
    return [ref.path(c) for c in ref.CONTRACTS]


def test_both_variants_are_built_and_current(built):
    for so in built:
        assert os.path.isfile(so), so
    up_to_date = subprocess.run(["make", "-q", "-C", os.path.join(ROOT, "oracle"), "-f", "ref.mk", f"REF={os.path.abspath(oracle.reference_dir())}"],
                                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
    assert up_to_date == 0, "oracle/_ref/ is older than its recipe or its sources"
    assert not [f for f in os.listdir(ref.REF_DIR) if f.endswith((".s", ".ll", ".bc"))], "assembly or IR left in oracle/_ref/"


def test_exports_are_the_reference_ten(built):
    want = open(os.path.join(ROOT, "tests", "golden", "reference_mangled_symbols.txt")).read().split()
    for so in built:
        out = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], text=True)
        got = {ln.split()[-1] for ln in out.splitlines() if ln.split() and re.match(r"_Z\d+GPU", ln.split()[-1]) and " UND " not in ln}
        # the ten of the headers, plus the one helper GPUSolver.cu defines without declaring it (GPUCheckError, :20)
        assert got == set(want) | {"_Z13GPUCheckErrorPc"}, f"{so}: {sorted(got ^ set(want))}"


def test_internal_calls_bind_to_the_reference_itself(built):
    """librtdd.so exports the same ten names (csrc/dropin.cpp); -Wl,-Bsymbolic keeps the reference's calls into itself inside it."""
    for so in built:
        out = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-d", so], text=True)
        assert re.search(r"\(FLAGS\)\s+.*\bSYMBOLIC\b", out), f"{so} is not linked -Bsymbolic:\n{out}"


def test_nothing_of_the_reference_is_tracked():
    if not os.path.isdir(os.path.join(ROOT, ".git")) or shutil.which("git") is None:
        pytest.skip("not a git checkout")
    assert subprocess.check_output(["git", "-C", ROOT, "ls-files", "oracle/_ref"], text=True).strip() == ""
    for f in ("oracle/_ref/", "oracle/_ref/libref_c0.so", "oracle/_ref/GPUSolver.hip"):
        assert subprocess.run(["git", "-C", ROOT, "check-ignore", "-q", f]).returncode == 0, f"{f} is not git-ignored"


# ---- the contraction of each build, on its ISA ------------------------------------------------------------------------------------
def _disassemble(so, tmp):
    """{mangled function: [(mnemonic, [operands])]} of the gfx950 code objects inside `so`, unpacked into `tmp` (never into the tree)."""
    local = os.path.join(tmp, os.path.basename(so))
    shutil.copy(so, local)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, stdout=subprocess.DEVNULL)
    objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f)
    assert objs, f"no gfx950 code object in {so}"
    funcs, cur = {}, None
    for o in objs:
        for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", o], text=True).splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
            if m:
                cur = funcs.setdefault(m.group(1), [])
            elif cur is not None and line.startswith(("\t", " ")) and line.strip():
                text = line.split("//")[0].strip()
                if text:
                    mn, _, ops = text.partition(" ")
                    cur.append((mn, [o.strip().lstrip("-") for o in ops.split(",") if o.strip()]))
    return funcs


def _kernel(funcs, name):
    hits = [k for k in funcs if name in k]
    assert len(hits) == 1, f"{name}: {hits}"
    return funcs[hits[0]]


def _outside_division(instrs):
    """The instructions outside every v_div_scale_f32 .. v_div_fixup_f32 span (the correctly rounded f32 division's own fmas)."""
    out, inside = [], False
    for mn, ops in instrs:
        if mn.startswith("v_div_scale_f32"):
            inside = True
        if not inside:
            out.append((mn, ops))
        if mn.startswith("v_div_fixup_f32"):
            inside = False
    return out


def _fused(instrs):
    """[(multiplicands, addend)] of the f32 fma-class instructions; v_fmac's addend is its destination, v_fmamk's is its last
    operand (d = s0 * K + s1), v_fmaak's a literal (d = s0 * s1 + K)."""
    out = []
    for mn, ops in instrs:
        if not mn.startswith(FMA):
            continue
        out.append(({ops[1], ops[2]}, ops[0] if mn.startswith("v_fmac_f32") else ops[3]))
    return out


def _dest(instrs, prefix, pred=lambda ops: True):
    hits = [ops[0] for mn, ops in instrs if mn.startswith(prefix) and pred(ops)]
    assert hits, f"no {prefix}"
    return hits[-1]


@pytest.fixture(scope="module")
def isa(built, tmp_path_factory):
    return {c: _disassemble(ref.path(c), str(tmp_path_factory.mktemp(f"isa_c{c}"))) for c in ref.CONTRACTS}


def test_solver_contraction_matches_the_oracle_variants(isa):
    """matrixFreeSolver (src/GPUSolver.cu:73-106, 226-262): c0 fuses nothing of the source's arithmetic (its only fmas are the
    correctly rounded division's), c1 fuses exactly the oracle's six (rtdd_oracle.c mean4 / orc_sweep): the four `sum += w*x`, the
    Chebyshev `gamma*(r-x)+x` and `omega*(..)+prev`.  No v_pk_add_f32 in c1: the sum/count additions are not paired into packed adds
    (which would leave the four products unfused: the reason for -fno-slp-vectorize)."""
    k0, k1 = _kernel(isa[0], "matrixFreeSolver"), _kernel(isa[1], "matrixFreeSolver")
    f0, f1 = _fused(_outside_division(k0)), _fused(_outside_division(k1))
    assert len(f0) == 0, f"c0 matrixFreeSolver fuses {len(f0)} operations of the source (expected none)"
    assert len(f1) == 6, f"c1 matrixFreeSolver fuses {len(f1)} operations of the source (expected 4 x sum, gamma, omega = 6)"
    assert not [mn for mn, _ in k1 if mn.startswith("v_pk_add_f32")], "c1 matrixFreeSolver pairs sum/count into v_pk_add_f32"
    assert len(_fused(k1)) - len(_fused(k0)) == 6


def test_desaturation_fuses_the_left_product(isa):
    """simulateDesaturation (src/GPUDepthEffect.cu:22-25) `f * gray + (1 - f) * orig`: c1 fuses the LEFT product,
    fma(f, gray, (1-f)*orig), one per channel -- the oracle's orc_desaturate and the product's desat_px<true>; c0 fuses none."""
    for c in ref.CONTRACTS:
        k = _outside_division(_kernel(isa[c], "simulateDesaturation"))
        f = _dest(_kernel(isa[c], "simulateDesaturation"), "v_div_fixup_f32")    # f = depth / 255.0 (binary32, correctly rounded)
        one_minus_f = _dest(k, "v_sub_f32", lambda ops: ops[1] == "1.0" and ops[2] == f)
        blend = [(m, a) for m, a in _fused(k) if f in m | {a} or one_minus_f in m | {a}]
        if c == 0:
            assert blend == [], f"c0 simulateDesaturation fuses {blend}"
        else:
            assert len(blend) == 3, f"c1 simulateDesaturation: {len(blend)} fused blends, expected one per channel"
            for m, a in blend:
                assert f in m and one_minus_f not in m, f"c1 simulateDesaturation fuses the right product (1-f)*orig: {m} + {a}"


def test_haze_fuses_the_left_product(isa):
    """simulateHaze (src/GPUDepthEffect.cu:88-91) `t * orig + (1 - t) * 255`: c1 fuses the LEFT product, fma(t, orig, (1-t)*255), one
    per channel -- the oracle's orc_haze and the product's haze_px<true>; c0 fuses none of the three (the expf expansion's own fmas
    aside, which come before t exists)."""
    for c in ref.CONTRACTS:
        k = _outside_division(_kernel(isa[c], "simulateHaze"))
        t = _dest(k, "v_ldexp_f32")                                         # t = expf(..): the last step of the device expf
        after = k[max(i for i, (mn, _) in enumerate(k) if mn.startswith("v_ldexp_f32")):]
        blend = [(m, a) for m, a in _fused(after) if t in m | {a}]
        if c == 0:
            assert blend == [], f"c0 simulateHaze fuses {blend}"
        else:
            assert len(blend) == 3, f"c1 simulateHaze: {len(blend)} fused blends, expected one per channel"
            for m, a in blend:
                assert t in m and a != t, f"c1 simulateHaze does not fuse t*orig: {m} + {a}"
