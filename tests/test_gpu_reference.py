"""The product against the reference's OWN GPU code (-m gpu): oracle/_ref/libref_c{0,1}.so, the reference's three .cu files hipified
and built for gfx950 by build() (oracle/ref.mk; loader oracle/ref.py), run on identical device inputs next to librtdd.so.

Everything else in the suite ends at the CPU oracle, our own restatement of the reference; a misreading shared by the oracle and the
product passes there.  Here the reference decides.  RTDD_OPT_FP_CONTRACT = 0 is compared with libref_c0.so (-ffp-contract=off) and = 1
with libref_c1.so (every a*b+c the source writes fused, tests/test_reference_build.py pins which), bit for bit -- except haze, whose
reference calls the device expf (ocml here, libdevice on CUDA) where the product uses a deterministic, correctly rounded exp; see
HAZE_* below.  Depths stay in [0, 255]: the reference's float -> unsigned char casts are undefined outside it (oracle/ref.py).
Skipped, with the reason, when build() had no reference tree to build oracle/_ref/ from."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from cascade_ref import pyramid_levels
from dataset_util import PAIRS, load_pair
from golden_util import sha
from gpu_util import assert_bit_equal, down, up
from oracle import ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libref_c0.so / libref_c1.so not built "
                                                  "(build() found no reference tree; tests/test_reference_build.py)")]
CONTRACTS = ref.CONTRACTS
# Haze: the device expf the reference calls differs from the correctly rounded exp on a fraction of the arguments
# (float)(-2d / 255.0), d in [0, 255].  Measured on gfx950 over 2^24 + 1 depths uniform in value: c0 6.37 % (never by more than 1 ulp),
# c1 28.1 % (its expf expansion is contracted too; 0.45 % by 2 ulps); never at d = 0 or 255.  An output byte can only differ where t
# does, and then -- t * orig + (1 - t) * 255 moves by < 255 * 2 ulp -- by one grey level at most; so the fraction of differing bytes is
# bounded by that rate, plus binomial slack for the number of pixels a test draws.
HAZE_EXPF_DIFF_RATE = {0: 0.0637, 1: 0.281}


@pytest.fixture(scope="module")
def refs():
    return {c: ref.RefLib(c) for c in CONTRACTS}


@pytest.fixture(scope="module")
def _ctx():
    c = rt.Context(0)
    yield c
    c.close()


@pytest.fixture
def ctx(_ctx):
    """The product's context with every option at its default and the reference's LUT (beta 0.4)."""
    _ctx.set_option(rt.OPT_FP_CONTRACT, 1); _ctx.set_option(rt.OPT_PERSISTENT, 1)
    for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH, rt.OPT_ROWS_PER_WAVE, rt.OPT_DEFOCUS_PATH):
        _ctx.set_option(k, 0)
    _ctx.GPULoadWeights(0.4)
    return _ctx


@pytest.fixture(autouse=True)
def _no_reference_errors(capfd):
    """The reference reports a failed launch or call only by printing `GPU<name>: <error>` (src/GPUSolver.cu:20-26)."""
    yield
    out = capfd.readouterr().out
    assert not ref.ERROR_LINE.search(out), f"the reference reported an error:\n{out}"


def pitched(a, pad):
    """A device copy of `a` whose rows are `pad` pixels longer than the image: a pitch that is not cols x pixel size."""
    import torch
    a = np.ascontiguousarray(a)
    base = torch.zeros((a.shape[0], a.shape[1] + pad) + a.shape[2:], dtype=torch.from_numpy(a[:0]).dtype, device="cuda:0")
    view = base[:, :a.shape[1]]
    view.copy_(torch.from_numpy(a).to("cuda:0"))
    return view


def _bgr(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


# ---- GPUMatrixFreeSolver ---------------------------------------------------------------------------------------------------------
def edge_problem(rows, cols, seed):
    """(depth, scribble, gray) aimed at the solver's edges:
    gray -- random, so neighbour differences cover 0..255 (LUT entries 219..255 are denormal at beta 0.4), and a band of a 0/255
            checkerboard whose pixels have four denormal weights (four zero weights at beta 1.0: count == 0);
    depth -- by row: random in [0, 255]; (uchar) steps of exactly 4 and of 5 between horizontal neighbours; 99 next to the float just
            below 104 ((uchar) 103: a step of 4 that a rounding cast would make 5); 100.25 next to 100.75 (one (uchar) value);
            plus 0, 255 and the float just below 255;
    scribble -- values 0..254 (not scribbled) with 255 on ~6% of the pixels, a whole row and a whole column."""
    rng = np.random.default_rng(seed)
    x = np.arange(cols)[None, :] % 2
    gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    band = slice(rows // 3, rows // 3 + max(1, rows // 8))
    gray[band] = (((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2) * 255).astype(np.uint8)[band]
    below104, below255 = np.nextafter(np.float32(104), np.float32(0)), np.nextafter(np.float32(255), np.float32(0))
    rows_of = [rng.uniform(0, 255, (1, cols)), 100 + 4 * x, 100 + 5 * x, np.where(x == 1, below104, np.float32(99)),
               np.where(x == 1, 100.75, 100.25), np.where(x == 1, below255, 255.0) * (np.arange(cols)[None, :] % 3 != 2)]
    depth = np.concatenate([np.broadcast_to(rows_of[y % len(rows_of)], (1, cols)) for y in range(rows)]).astype(np.float32)
    scribble = rng.integers(0, 255, (rows, cols), dtype=np.uint8)
    scribble[rng.random((rows, cols)) < 0.06] = 255
    if rows >= 3 and cols >= 3:
        scribble[rows // 2, :] = 255; scribble[:, cols // 2] = 255
    assert depth.min() >= 0 and depth.max() <= 255
    return depth, scribble, gray


def _solve(lib_or_ctx, problem, rows, cols, beta, iters, level, pads):
    depth, scribble, gray = problem
    d, s, g = pitched(depth, pads[0]), pitched(scribble, pads[1]), pitched(gray, pads[2])
    lib_or_ctx.GPUMatrixFreeSolver(d, s, g, rows, cols, beta, iters, 1e-5, level)
    if isinstance(lib_or_ctx, rt.Context):
        lib_or_ctx.synchronize()
    return down(d)


def compare_solver(ctx, lib, problem, beta, iters_list, levels, opts=None, pads=(5, 3, 1)):
    rows, cols = problem[0].shape
    ctx.set_option(rt.OPT_FP_CONTRACT, lib.contract)
    for k, v in (opts or {}).items():
        ctx.set_option(k, v)
    ctx.GPULoadWeights(beta); lib.GPULoadWeights(beta)
    for level, max_level in levels:
        with lib.allocated(rows << level, cols << level, max_level + 1):
            ctx.GPUAllocateDeviceMemory(rows << level, cols << level, max_level + 1)
            for iters in iters_list:
                want = _solve(lib, problem, rows, cols, beta, iters, level, pads)
                got = _solve(ctx, problem, rows, cols, beta, iters, level, pads)
                assert_bit_equal(got, want, f"solver {rows}x{cols} level {level}/{max_level} {iters} sweeps beta {beta} contract {lib.contract} "
                                            f"{opts or 'default'} vs the reference")


ITERS = (0, 1, 2, 9, 10, 11, 12, 37)                     # the omega switch at S = 10, both result buffers
LEVELS = ((0, 0), (0, 2), (1, 2), (2, 2))                 # gray-only top level; threshold 0 at level 0; threshold 4 in between


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (15, 17), (16, 16), (17, 33), (67, 120), (135, 241), (270, 481)])
def test_solver_matches_the_reference(ctx, refs, shape, contract):
    compare_solver(ctx, refs[contract], edge_problem(*shape, seed=shape[0] * 31 + shape[1]), 0.4, ITERS, LEVELS)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("shape", [(1, 1), (15, 17), (67, 120)])
def test_solver_with_zero_weights_matches_the_reference(ctx, refs, shape, contract):
    """beta 1.0: LUT entries from 104 on are exactly 0, so the checkerboard band has count == 0 (src/GPUSolver.cu:103)."""
    compare_solver(ctx, refs[contract], edge_problem(*shape, seed=7), 1.0, (1, 10, 37), LEVELS)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("opts", [{rt.OPT_SWEEP_KERNEL: 1}, {rt.OPT_SWEEP_KERNEL: 2, rt.OPT_PERSISTENT: 0},
                                  {rt.OPT_SWEEP_KERNEL: 2, rt.OPT_PERSISTENT: 1}, {rt.OPT_SWEEP_KERNEL: 2, rt.OPT_TILE: 14}],
                         ids=["one-sweep", "blocked", "persistent", "column"])
@pytest.mark.parametrize("shape", [(17, 33), (135, 241), (270, 481)])
def test_solver_kernels_match_the_reference(ctx, refs, shape, opts, contract):
    """The product's sweep kernels that tests/test_gpu_parity.py covers against the oracle, here against the reference."""
    compare_solver(ctx, refs[contract], edge_problem(*shape, seed=shape[1]), 0.4, (9, 10, 11, 37), LEVELS, opts=opts)


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("shape,iters", [((1080, 1920), 1000), ((2160, 3840), 100)])
def test_solver_full_size_matches_the_reference(ctx, refs, shape, iters, contract):
    compare_solver(ctx, refs[contract], edge_problem(*shape, seed=5), 0.4, (iters,), ((0, 0),), pads=(0, 64, 0))


# ---- image kernels (integer only: both builds must agree) ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (853, 1280)])
def test_convert_to_float_matches_the_reference(ctx, refs, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows + cols)
    src = _bgr(rows, cols, 3); mask = np.where(rng.random(shape) < 0.3, 255, rng.integers(0, 255, shape)).astype(np.uint8)
    dst = rng.uniform(0, 255, shape).astype(np.float32)
    outs = []
    for lib in [refs[c] for c in CONTRACTS] + [ctx]:
        d = pitched(dst, 3)
        lib.GPUConvertToFloat(pitched(src, 1), d, pitched(mask, 2), rows, cols)
        if lib is ctx:
            ctx.synchronize()
        outs.append(down(d))
    for got in outs[1:]:
        assert_bit_equal(got, outs[0], f"GPUConvertToFloat {shape}")


@pytest.mark.parametrize("density", [0.02, 0.6])
@pytest.mark.parametrize("prev,curr", [((16, 16), (8, 8)), ((17, 33), (8, 16)), ((2, 17), (1, 8)), ((17, 2), (8, 1)), ((1, 9), (1, 4)),
                                       ((9, 1), (4, 1)), ((853, 1280), (426, 640)), ((1706, 2560), (853, 1280))])
def test_pyrdown_annotation_matches_the_reference(ctx, refs, prev, curr, density):
    rng = np.random.default_rng(prev[0] * prev[1])
    pm = np.where(rng.random(prev) < density, 255, 32).astype(np.uint8); pe = _bgr(*prev, 4)
    cm = np.where(rng.random(curr) < 0.1, 255, 32).astype(np.uint8); ce = _bgr(*curr, 5)     # stale state: never cleared
    outs = []
    for lib in [refs[c] for c in CONTRACTS] + [ctx]:
        gm, ge = pitched(cm, 3), pitched(ce, 1)
        lib.GPUPyrDownAnnotation(pitched(pm, 1), pitched(pe, 2), *prev, gm, ge, *curr)
        if lib is ctx:
            ctx.synchronize()
        outs.append((down(gm), down(ge)))
    for gm, ge in outs[1:]:
        assert np.array_equal(gm, outs[0][0]) and np.array_equal(ge, outs[0][1]), f"GPUPyrDownAnnotation {prev} -> {curr}"


@pytest.mark.parametrize("x,y,r", [(50, 40, 21), (0, 0, 9), (99, 79, 10), (-5, 30, 20), (300, 300, 8), (10, 10, 0), (10, 10, 1), (20, 20, -6)])
def test_paint_image_matches_the_reference(ctx, refs, x, y, r):
    rows, cols = 80, 100
    e = _bgr(rows, cols, 7); m = np.full((rows, cols), 32, np.uint8)
    outs = []
    for lib in [refs[c] for c in CONTRACTS] + [ctx]:
        ge, gm = pitched(e, 1), pitched(m, 3)
        lib.GPUPaintImage(x, y, 192, r, ge, gm, rows, cols)
        if lib is ctx:
            ctx.synchronize()
        outs.append((down(ge), down(gm)))
    for ge, gm in outs[1:]:
        assert np.array_equal(ge, outs[0][0]) and np.array_equal(gm, outs[0][1]), f"GPUPaintImage {(x, y, r)}"


# ---- depth effects ---------------------------------------------------------------------------------------------------------------
def _effect(lib, name, orig, depth, gray=None):
    rows, cols = depth.shape
    art = pitched(np.zeros_like(orig), 2)
    o, d = pitched(orig, 1), pitched(depth, 3)
    if name == "desaturation":
        lib.GPUSimulateDesaturation(o, pitched(gray, 5), d, art, rows, cols)
    elif name == "defocus":
        lib.GPUSimulateDefocus(o, d, art, rows, cols)
    else:
        lib.GPUSimulateHaze(o, d, art, rows, cols)
    if isinstance(lib, rt.Context):
        lib.synchronize()
    return down(art)


def _depths(rows, cols, seed):
    d = np.random.default_rng(seed).uniform(0, 255, (rows, cols)).astype(np.float32)
    d[::7, ::5] = 255.0; d[1::7, ::5] = 0.0
    return d


def assert_haze_close(got, want, depth, contract, what):
    """Bytes equal where depth is 0 or 255 (t = 1 and expf(-2): no disagreement there); elsewhere at most one grey level apart on at
    most the measured expf disagreement rate of the values."""
    ends = (depth == 0) | (depth == 255)
    assert np.array_equal(got[ends], want[ends]), f"{what}: haze differs at depth 0 / 255"
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert diff.max() <= 1, f"{what}: haze differs by {diff.max()} grey levels"
    frac, rate = float((diff != 0).mean()), HAZE_EXPF_DIFF_RATE[contract]
    bound = rate + 4 * np.sqrt(rate * (1 - rate) / depth.size)
    assert frac <= bound, f"{what}: {frac:.4f} of the haze bytes differ (bound {bound:.4f})"


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (135, 241), (1080, 1920)])
def test_desaturation_and_haze_match_the_reference(ctx, refs, shape, contract):
    rows, cols = shape
    orig, depth, gray = _bgr(rows, cols, 11), _depths(rows, cols, 31), _bgr(rows, cols, 12)[..., 0].copy()
    ctx.set_option(rt.OPT_FP_CONTRACT, contract)
    want = _effect(refs[contract], "desaturation", orig, depth, gray)
    assert np.array_equal(_effect(ctx, "desaturation", orig, depth, gray), want), f"desaturation {shape} contract {contract}"
    assert_haze_close(_effect(ctx, "haze", orig, depth), _effect(refs[contract], "haze", orig, depth), depth, contract, f"haze {shape} contract {contract}")


def defocus_depths(rows, cols, seed):
    """Random depths, and depths where kernelSize * d / 255.0 (src/GPUDepthEffect.cu:43) lands exactly on an integer or one ulp of d
    either side of it -- windows of 0 and 1 included (count == 0: the pixel is copied)."""
    k = int(0.025 * float(np.sqrt(np.float32(rows * rows + cols * cols))))
    on = np.array([np.float32(255.0 * n / k) for n in range(k + 1)] if k else [np.float32(0)], np.float32)
    cands = np.concatenate([on, np.nextafter(on, np.float32(0)), np.nextafter(on, np.float32(256))])
    cands = cands[(cands >= 0) & (cands <= 255)]
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    pick = rng.random((rows, cols)) < 0.5
    d[pick] = rng.choice(cands, int(pick.sum()))
    return d


@pytest.mark.parametrize("shape,path", [((1, 7), 0), ((17, 33), 0), ((135, 241), 0), ((270, 481), 0), ((1080, 1920), 0),
                                        ((135, 241), 1), ((270, 481), 1), ((135, 241), 2), ((270, 481), 2)])
def test_defocus_matches_the_reference(ctx, refs, shape, path):
    """Every table path of the product's defocus (RTDD_OPT_DEFOCUS_PATH) at the small sizes; the default one at 1080p."""
    rows, cols = shape
    orig, depth = _bgr(rows, cols, 13), defocus_depths(rows, cols, 17)
    want = [_effect(refs[c], "defocus", orig, depth) for c in CONTRACTS]
    assert np.array_equal(want[0], want[1]), "the reference's two builds disagree on defocus (integer sums, one division)"
    ctx.set_option(rt.OPT_DEFOCUS_PATH, path)
    assert np.array_equal(_effect(ctx, "defocus", orig, depth), want[0]), f"defocus {shape} path {path}"


# ---- the ten functions in src/main.cpp's order, and the committed goldens -------------------------------------------------------
def main_sequence(lib, oracle, bgr, ann, contract, paints=(), max_iterations=1000):
    """src/main.cpp's depth estimate and effects on one library's ten functions: GPUAllocateDeviceMemory (:149), GPULoadWeights (:155),
    GPUPaintImage (:56), GPUPyrDownAnnotation per level (:249), GPUConvertToFloat (:257), per level GPUMatrixFreeSolver (:266) with
    pyrUp + GPUConvertToFloat between levels (:272-281), the three effects (:192-220), GPUFreeDeviceMemory (:336).  The OpenCV steps
    (gray pyramid, pyrUp) are the oracle's restatements on the host (tests/cascade_ref.py).  Returns every intermediate."""
    rows, cols = bgr.shape[:2]
    P = pyramid_levels(rows, cols)
    sizes = [ref.level_shape(rows, cols, l) for l in range(P)]
    gray = [oracle.bgr2gray(bgr)]
    for l in range(1, P):
        gray.append(oracle.pyrdown_u8(gray[-1]))
    out = {"sizes": sizes, "depth": [None] * P}
    with lib.allocated(rows, cols, P):
        lib.GPULoadWeights(0.4)
        edited = [up(np.zeros(s + (3,), np.uint8)) for s in sizes]; scribble = [up(np.zeros(s, np.uint8)) for s in sizes]
        depth = [up(np.full(s, 255.0, np.float32)) for s in sizes]
        g = [up(x) for x in gray]
        e0 = bgr.copy(); lab = ann != 32; e0[lab] = ann[lab][:, None]                     # main.cpp:160-168
        edited[0] = up(e0); scribble[0] = up(np.where(lab, 255, ann).astype(np.uint8))
        for x, y, label, radius in paints:
            lib.GPUPaintImage(x, y, label, radius, edited[0], scribble[0], rows, cols)
        for l in range(1, P):
            lib.GPUPyrDownAnnotation(scribble[l - 1], edited[l - 1], *sizes[l - 1], scribble[l], edited[l], *sizes[l])
        lib.GPUConvertToFloat(edited[P - 1], depth[P - 1], scribble[P - 1], *sizes[P - 1])
        for l in range(P - 1, -1, -1):
            iters = int(np.float32(max_iterations) / np.float32(2.0) ** ((P - 1) - l))
            lib.GPUMatrixFreeSolver(depth[l], scribble[l], g[l], *sizes[l], 0.4, iters, 1e-5, l)
            out["depth"][l] = down(depth[l])
            if l > 0:
                depth[l - 1] = up(oracle.pyrup_f32(out["depth"][l], *sizes[l - 1], contract=contract))
                lib.GPUConvertToFloat(edited[l - 1], depth[l - 1], scribble[l - 1], *sizes[l - 1])
        out["scribble"] = [down(s) for s in scribble]; out["edited"] = [down(e) for e in edited]
        orig = up(bgr); art = up(np.zeros_like(bgr))
        lib.GPUSimulateDefocus(orig, depth[0], art, rows, cols); out["defocus"] = down(art)
        lib.GPUSimulateDesaturation(orig, g[0], depth[0], art, rows, cols); out["desaturation"] = down(art)
        lib.GPUSimulateHaze(orig, depth[0], art, rows, cols); out["haze"] = down(art)
    return out


@pytest.fixture
def dropin():
    """librtdd.so's ten mangled entry points (csrc/dropin.cpp: what an unchanged main.cpp links against), driven like the reference;
    RTDD_OPT_FP_CONTRACT is set on the shim's process-global context and put back afterwards."""
    L = rt.lib()
    L.rtdd_dropin_context.restype = C.c_void_p
    h = C.c_void_p(L.rtdd_dropin_context())
    assert h.value

    def make(contract):
        assert L.rtdd_set_option(h, C.c_int(rt.OPT_FP_CONTRACT), C.c_int(contract)) == 0
        return ref.RefLib(contract, library=L)
    yield make
    L.rtdd_set_option(h, C.c_int(rt.OPT_FP_CONTRACT), C.c_int(1))


@pytest.mark.parametrize("contract", CONTRACTS)
@pytest.mark.parametrize("rows,cols", [(270, 481), (624, 672)])
def test_all_ten_functions_in_main_cpp_order_match_the_reference(oracle, refs, dropin, rows, cols, contract):
    """tests/test_gpu_dropin.py's sequence, with the reference itself on the other side instead of the oracle."""
    from test_gpu_cascade import _bgr as scene
    bgr, ann = scene(rows, cols, 21)
    paints = [(cols // 3, rows // 2, 192, 9), (cols // 2, rows // 3, 0, 12)]
    want = main_sequence(refs[contract], oracle, bgr, ann, contract, paints)
    got = main_sequence(dropin(contract), oracle, bgr, ann, contract, paints)
    P = len(want["sizes"])
    for l in range(P):
        assert np.array_equal(got["scribble"][l], want["scribble"][l]) and np.array_equal(got["edited"][l][..., 0], want["edited"][l][..., 0]), \
            f"annotation pyramid level {l}"
    for l in range(P - 1, -1, -1):                                     # coarsest first: the first level that differs is the one to read
        assert_bit_equal(got["depth"][l], want["depth"][l], f"contract {contract} depth level {l} of {P}")
    assert np.array_equal(got["defocus"], want["defocus"]), "defocus"
    assert np.array_equal(got["desaturation"], want["desaturation"]), "desaturation"
    assert_haze_close(got["haze"], want["haze"], got["depth"][0], contract, "haze")


@pytest.mark.parametrize("contract", CONTRACTS)
def test_the_reference_reproduces_the_dataset_goldens(oracle, refs, contract):
    """The twelve pairs of tests/golden/dataset/ through the reference's own kernels (main.cpp order, OpenCV steps restated): every
    level's depth hash equals manifest.json's depth_sha_c{contract} -- hashes the oracle wrote; the effects' hashes (recorded on the
    contracted cascade) likewise, haze within the expf bound of the oracle's.  The goldens are then the reference's, not only ours."""
    for name in PAIRS:
        bgr, ann, e = load_pair(name)
        got = main_sequence(refs[contract], oracle, bgr, ann, contract)
        assert [list(s) for s in got["sizes"]] == e["sizes"]
        for l in range(len(got["sizes"]) - 1, -1, -1):
            assert sha(got["depth"][l]) == e[f"depth_sha_c{contract}"][l], f"{name} contract {contract}: level {l} differs from the golden"
        assert sha(oracle.depth_to_u8(got["depth"][0])) == e[f"depth_u8_sha_c{contract}"], f"{name} depth_u8"
        if contract == 1:                                              # the manifest's effects are of the contracted cascade's depth
            assert sha(got["defocus"]) == e["defocus_sha"], f"{name} defocus"
            assert sha(got["desaturation"]) == e["desaturate_sha"], f"{name} desaturation"
            assert_haze_close(got["haze"], oracle.haze(bgr, got["depth"][0], 1), got["depth"][0], 1, f"{name} haze")
