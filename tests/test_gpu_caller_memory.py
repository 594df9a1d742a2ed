"""How every entry point of the C ABI touches the CALLER's memory (-m gpu): each image of a call is a sub-image view (tests/roi_util.py: a
base pointer of any alignment class, any row stride, foreign bytes all around), and each image's layout varies INDEPENDENTLY of the
others' -- the alignment predicates of the launchers are per image.  After every call

  * every output's pixels equal the reference, bit for bit -- the references the suite already trusts (the oracle, the numpy
    restatements), computed ONCE per shape: the expected output does not depend on the layout;
  * every byte of an output's parent outside the view still holds its fill (Roi.result());
  * every input's parent, view included, is bit-identical to what was uploaded (Roi.assert_unchanged()).

Layouts: LAYOUTS_U8 and LAYOUTS_F32 have 7 entries each.  A call with two images runs the full product (49); a call with three images
(343) or four (2401) runs 49 combinations in which every layout of every image and every PAIR of layouts of any two images occurs
(roi_util.covering: rows of an orthogonal array); what is dropped are the triples and quadruples that no pair distinguishes.  The two
values of RTDD_OPT_FP_CONTRACT run on the solver's first combination only (the layout dispatch does not depend on contraction).

Shapes: (9, 67), (13, 131), (5, 259), (1, 7), (7, 1), (2, 2) -- a ragged last group of four, a ragged 64-pixel strip, a ragged 256-pixel
workgroup, more than one 4-row group and 8-row lookup tile, one and two columns and rows -- and (70, 133) for the solver (a 64 x 64 tile
crossed both ways).  rtdd_pyrup_depth adds (9, 66) and (5, 130): its four-pixel kernel needs a destination width that is a multiple of 4.
Solver levels: 0 of 1 and 1 of 2 (both the un-gated rule) and, for the reference's scheme, 1 of 3: the GATED rule, which reads depth row
y + 1 (gated = level != levels - 1).

An f32 image whose pointer or pitch is no multiple of 4 is illegal by contract (include/rtdd.h): test_f32_alignment_is_refused asserts
the refusal for every entry point that takes one, that nothing was written, and that the context still serves a legal call."""
import ctypes as C
import itertools

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import strokes_ref as sr
from cascade_ref import Cascade
from lens_blur_ref import lens_blur_by_row_prefixes
from refocus_ref import haze_ex, refocus_by_summed_area_table
from relight_ref import DIRECTIONAL, POINT, light, relight
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from shadow_ref import relight_shadowed, shadow
from stereo_ref import stereo

pytestmark = pytest.mark.gpu
SHAPES = [(9, 67), (13, 131), (5, 259), (1, 7), (7, 1), (2, 2)]
SOLVER_SHAPES = SHAPES + [(70, 133)]


@pytest.fixture(scope="module")
def ctx():
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        yield c


# ---- the machinery: images, layouts, one call per combination -------------------------------------------------------------------------
def _layouts(host):
    host = np.asarray(host)
    w = host.size // max(host.shape[0], 1) * host.itemsize
    return [(lead, pitch_for(w, lead, res)) for lead, res in (LAYOUTS_F32 if host.dtype == np.float32 else LAYOUTS_U8)]


def _bits_equal(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _sweep(ctx, what, inputs, outputs, call, want, first_only=False):
    """inputs / outputs: {name: host image} (an output's host image is what it holds before the call: zeros, or its in/out content).
    call(images): queues the entry point on ctx with images[name] = (pointer, pitch).  want: {output name: expected pixels}.
    One call per combination of layouts (every pair of layouts of any two images); returns the number of calls."""
    names = list(inputs) + list(outputs)
    hosts = {**inputs, **outputs}
    lay = {n: _layouts(hosts[n]) for n in names}
    ins = {n: [Roi(inputs[n], lead, pitch, FILL_INPUT, what=f"{what}: input {n} (lead {lead}, pitch {pitch})") for lead, pitch in lay[n]] for n in inputs}
    combos = covering(*[len(lay[n]) for n in names])
    assert len(combos) >= max(len(v) for v in lay.values())
    if first_only:
        combos = combos[:1]
    for k, combo in enumerate(combos):
        pick = dict(zip(names, combo))
        outs = {n: Roi(outputs[n], *lay[n][pick[n]], FILL_OUTPUT, seed=k, what=f"{what}: output {n} (lead {lay[n][pick[n]][0]}, pitch {lay[n][pick[n]][1]})")
                for n in outputs}
        images = {n: ins[n][pick[n]].img for n in inputs}
        images.update({n: outs[n].img for n in outputs})
        call(images)
        ctx.synchronize()
        where = f"{what}, layouts " + ", ".join(f"{n} {lay[n][pick[n]]}" for n in names)
        for n in outputs:
            got = outs[n].result()
            if not _bits_equal(got, want[n]):
                differ = np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want[n]).view(np.uint8)
                raise AssertionError(f"{where}: output {n} differs from the reference in {int(differ.sum())} of {differ.size} bytes")
        for n in inputs:
            ins[n][pick[n]].assert_unchanged()
    return len(combos)


def _rgb(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def _u8(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def _mask(rows, cols, seed):
    """255 (the Dirichlet label) on ~15 % of the pixels, at least one; 254 and 0 on others (only 255 counts), 32 elsewhere."""
    rng = np.random.default_rng(seed)
    u = rng.random((rows, cols))
    m = np.where(u < 0.15, 255, np.where(u < 0.25, 254, np.where(u < 0.3, 0, 32))).astype(np.uint8)
    m[rows // 2, cols // 2] = 255
    return m


def _depth01(rows, cols, seed):
    """A depth map in [0, 255] with exact 0 and 255."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.1] = 255.0
    d[rng.random((rows, cols)) < 0.1] = 0.0
    return d


def _problem(rows, cols, seed):
    rng = np.random.default_rng(seed)
    gray = (_u8(rows, cols, seed) // 4 + 90).astype(np.uint8)
    gray[rng.random((rows, cols)) < 0.2] = 7                     # some strong edges, denormal weights included
    mask = _mask(rows, cols, seed + 1)
    depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    lab = rng.integers(0, 255, (rows, cols)).astype(np.float32)
    depth[mask == 255] = lab[mask == 255]
    return depth, mask, gray


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
def _solver_reference(oracle, lut, method, depth, mask, gray, level, levels, contract):
    x = depth.copy()
    if method == "jacobi":
        return oracle.solve(x, mask, gray, 9, level, levels - 1, lut, contract)
    idx = oracle.index_to_weight(gray, depth, level, levels - 1)
    if method == "rbgs":
        for _ in range(9):
            oracle.rbgs_sweep(x, idx, mask, lut, contract)
    else:
        oracle.mg_solve(x, idx, mask, lut, contract, 2, 0.0, 1)
    return x


def _solver_call(ctx, entry, rows, cols, level):
    def call(im):
        if entry == "matrix_free":
            ctx.GPUMatrixFreeSolver(im["depth"], im["scribble"], im["gray"], rows, cols, 0.4, 9, 0.0, level)
        elif entry == "rbgs":
            assert ctx.solve_ex(im["depth"], im["scribble"], im["gray"], rows, cols, level, method=rt.METHOD_RED_BLACK_GS, maxIterations=9)[0] == 9
        elif entry == "multigrid":
            assert ctx.solve_ex(im["depth"], im["scribble"], im["gray"], rows, cols, level, method=rt.METHOD_MULTIGRID, maxIterations=2)[0] == 2
        else:
            assert ctx.solve_ex(im["depth"], im["scribble"], im["gray"], rows, cols, level, maxIterations=9)[0] == 9
    return call


SOLVER_ENTRIES = [("matrix_free", "jacobi", 0), ("solve_ex kernel 1", "jacobi", 1), ("solve_ex kernel 2", "jacobi", 2), ("rbgs", "rbgs", 0),
                  ("multigrid", "multigrid", 0)]


@pytest.mark.parametrize("entry,method,kernel", SOLVER_ENTRIES, ids=[e[0].replace(" ", "_") for e in SOLVER_ENTRIES])
@pytest.mark.parametrize("shape", SOLVER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver(ctx, oracle, lut, shape, entry, method, kernel):
    """rtdd_matrix_free_solver, and rtdd_solve_ex with both sweep kernels, red-black Gauss-Seidel and multigrid: depth is input AND output
    -- the view equals the oracle, everything around it its fill; scribble and gray are untouched."""
    rows, cols = shape
    depth, mask, gray = _problem(rows, cols, 100 + rows)
    levels_of = [(0, 1), (1, 2)] + ([(1, 3)] if method == "jacobi" else [])
    calls = 0
    try:
        for level, levels in levels_of:
            ctx.GPUAllocateDeviceMemory(rows << level, cols << level, levels)
            ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel)
            for contract in (1, 0):
                ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                want = _solver_reference(oracle, lut, method, depth, mask, gray, level, levels, contract)
                calls += _sweep(ctx, f"{entry} {rows}x{cols} level {level} of {levels} contract {contract}", {"scribble": mask, "gray": gray}, {"depth": depth},
                                _solver_call(ctx, entry, rows, cols, level), {"depth": want}, first_only=contract == 0)
    finally:
        ctx.set_option(rt.OPT_SWEEP_KERNEL, 0); ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    assert calls == len(levels_of) * 50


def test_solver_smaller_problem_in_larger_allocation(ctx, oracle, lut):
    """(70, 133), then (9, 67) on the same context WITHOUT re-allocating, then (70, 133) again, all from views: every result is the
    oracle's -- nothing stale in the level's planes leaks into a smaller problem, nothing of the smaller one into the next."""
    ctx.GPUAllocateDeviceMemory(70, 133, 1)
    big, small = _problem(70, 133, 7), _problem(9, 67, 8)
    for k, (depth, mask, gray) in enumerate((big, small, big, small)):
        rows, cols = depth.shape
        want = oracle.solve(depth.copy(), mask, gray, 9, 0, 0, lut, 1)
        (ld, pd), (ls, ps), (lg, pg) = _layouts(depth)[(3 + k) % 7], _layouts(mask)[(1 + k) % 7], _layouts(gray)[(5 + k) % 7]
        d, s, g = Roi(depth, ld, pd, FILL_OUTPUT, seed=k, what="depth"), Roi(mask, ls, ps, what="scribble"), Roi(gray, lg, pg, what="gray")
        ctx.GPUMatrixFreeSolver(d.img, s.img, g.img, rows, cols, 0.4, 9, 0.0, 0)
        ctx.synchronize()
        assert _bits_equal(d.result(), want), f"solve {k} ({rows} x {cols})"
        s.assert_unchanged(); g.assert_unchanged()


# ---- index and image passes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_index_to_weight(ctx, oracle, shape):
    """The index buffer is dense, not an image: it sits inside a larger buffer whose other words must keep their pattern."""
    import torch
    rows, cols = shape
    depth, _, gray = _problem(rows, cols, 31)
    depth[::2, ::3] = np.random.default_rng(1).uniform(-20, 280, depth[::2, ::3].shape).astype(np.float32)
    n = rows * cols * 2
    for level, levels in ((0, 1), (0, 2), (1, 3)):
        ctx.GPUAllocateDeviceMemory(rows << level, cols << level, levels)
        want = oracle.index_to_weight(gray, depth, level, levels - 1)
        gs = [Roi(gray, l, p, what="gray") for l, p in _layouts(gray)]
        ds = [Roi(depth, l, p, what="depth") for l, p in _layouts(depth)]
        for g, d in itertools.product(gs, ds):
            buf = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            ctx.index_to_weight(g.img, d.img, buf[32:32 + n], level, rows, cols)
            ctx.synchronize()
            got = buf.cpu().numpy()
            assert (got[:32] == 0x5A5A5A5A).all() and (got[32 + n:] == 0x5A5A5A5A).all(), "index buffer: written outside"
            assert np.array_equal(got[32:32 + n].reshape(rows, cols, 2), want), (level, levels, g.what, d.what)
            g.assert_unchanged(); d.assert_unchanged()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_convert_to_float(ctx, oracle, shape):
    rows, cols = shape
    edited, mask = _rgb(rows, cols, 1), _mask(rows, cols, 2)
    dst = np.random.default_rng(3).uniform(0, 255, shape).astype(np.float32)
    want = oracle.convert_to_float(edited, dst.copy(), mask)
    assert _sweep(ctx, f"convert_to_float {shape}", {"src": edited, "mask": mask}, {"dst": dst},
                  lambda im: ctx.GPUConvertToFloat(im["src"], im["dst"], im["mask"], rows, cols), {"dst": want}) == 49


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyrdown_annotation(ctx, oracle, shape):
    """The shape is the COARSE (output) image's; the fine one is (2 r + 1, 2 c + 1).  Stale coarse state must survive."""
    crows, ccols = shape
    rows, cols = 2 * crows + 1, 2 * ccols + 1
    edited, mask = _rgb(rows, cols, 5), _mask(rows, cols, 6)
    cm, ce = np.where(_u8(crows, ccols, 7) < 20, 255, 0).astype(np.uint8), _rgb(crows, ccols, 8)
    wm, we = cm.copy(), ce.copy()
    oracle.pyrdown_annotation(mask, edited, wm, we)
    assert _sweep(ctx, f"pyrdown_annotation {shape}", {"prevScribble": mask, "prevEdited": edited}, {"currScribble": cm, "currEdited": ce},
                  lambda im: ctx.GPUPyrDownAnnotation(im["prevScribble"], im["prevEdited"], rows, cols, im["currScribble"], im["currEdited"], crows, ccols),
                  {"currScribble": wm, "currEdited": we}) == 49


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paint_image(ctx, oracle, shape):
    """Two stamps: one over the whole image and beyond every edge, one across the bottom-right corner."""
    rows, cols = shape
    e, m = _rgb(rows, cols, 7), np.full(shape, 32, np.uint8)
    stamps = [(cols // 2, rows // 2, 192, 2 * max(rows, cols) + 4), (cols - 1, rows - 1, 77, 5), (0, 0, 9, 1), (cols // 3, rows // 2, 130, 3)]
    we, wm = e.copy(), m.copy()
    for x, y, label, radius in stamps[1:]:
        oracle.paint_image(x, y, label, radius, we, wm)

    def some(im):
        for x, y, label, radius in stamps[1:]:
            ctx.GPUPaintImage(x, y, label, radius, im["edited"], im["scribble"], rows, cols)
    assert _sweep(ctx, f"paint_image {shape}", {}, {"edited": e, "scribble": m}, some, {"edited": we, "scribble": wm}) == 49
    x, y, label, radius = stamps[0]
    oracle.paint_image(x, y, label, radius, we, wm)
    assert (wm == 255).all()
    _sweep(ctx, f"paint_image over everything {shape}", {}, {"edited": e, "scribble": m},
           lambda im: (some(im), ctx.GPUPaintImage(x, y, label, radius, im["edited"], im["scribble"], rows, cols)), {"edited": we, "scribble": wm})


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paint_strokes(ctx, shape):
    rows, cols = shape
    orig = _rgb(rows, cols, 9)
    ed, scr = _rgb(rows, cols, 10), np.where(_u8(rows, cols, 11) < 40, 255, 0).astype(np.uint8)
    strokes = [(-3, rows // 2, cols + 3, rows // 2, 3, sr.BRUSH_SQUARE, 200), (cols // 2, -2, cols // 3, rows + 2, 4, sr.BRUSH_ROUND, sr.STROKE_ERASE),
               (cols - 1, rows - 1, cols - 1, rows - 1, 6, sr.BRUSH_ROUND, 17), (0, 0, cols // 4, rows - 1, 1, sr.BRUSH_SQUARE, 90),
               (cols - 2, 0, cols + 40, 0, 2, sr.BRUSH_SQUARE, sr.STROKE_ERASE)]
    we, ws = ed.copy(), scr.copy()
    sr.paint_strokes(strokes, we, ws, orig)
    assert (we != ed).any()
    assert _sweep(ctx, f"paint_strokes {shape}", {"original": orig}, {"edited": ed, "scribble": scr},
                  lambda im: ctx.paint_strokes(strokes, im["edited"], im["scribble"], rows, cols, original=im["original"]), {"edited": we, "scribble": ws}) == 49


# ---- depth effects --------------------------------------------------------------------------------------------------------------------------
def _zeros_like(a):
    return np.zeros_like(a)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blend_effects(ctx, oracle, shape):
    """rtdd_simulate_desaturation (four images), _haze and _haze_ex.  Haze against the oracle by the rule of test_gpu_kernels.py: equal bytes."""
    rows, cols = shape
    orig, gray, depth = _rgb(rows, cols, 11), _u8(rows, cols, 12), _depth01(rows, cols, 13)
    ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    assert _sweep(ctx, f"desaturation {shape}", {"original": orig, "gray": gray, "depth": depth}, {"artistic": _zeros_like(orig)},
                  lambda im: ctx.GPUSimulateDesaturation(im["original"], im["gray"], im["depth"], im["artistic"], rows, cols),
                  {"artistic": oracle.desaturate(orig, gray, depth, 1)}) == 49
    wild = depth.copy()
    wild[::2, ::3] = np.random.default_rng(3).uniform(-400, 700, wild[::2, ::3].shape).astype(np.float32)     # t > 1 and t -> 0
    _sweep(ctx, f"haze {shape}", {"original": orig, "depth": wild}, {"artistic": _zeros_like(orig)},
           lambda im: ctx.GPUSimulateHaze(im["original"], im["depth"], im["artistic"], rows, cols), {"artistic": oracle.haze(orig, wild, 1)})
    beta, air = 1.25, (200, 180, 90)
    _sweep(ctx, f"haze_ex {shape}", {"original": orig, "depth": depth}, {"artistic": _zeros_like(orig)},
           lambda im: ctx.simulate_haze_ex(im["original"], im["depth"], im["artistic"], rows, cols, beta, air),
           {"artistic": haze_ex(orig, depth, beta, air, 1, oracle.expf_det)})


def _with_path(ctx, path, fn):
    def call(im):
        ctx.set_option(rt.OPT_DEFOCUS_PATH, path)
        try:
            fn(im)
            assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == path
        finally:
            ctx.set_option(rt.OPT_DEFOCUS_PATH, 0)
    return call


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_defocus_family(ctx, oracle, shape, path):
    """rtdd_simulate_defocus and _refocus on the table (1) and the tile kernel (2), rtdd_simulate_lens_blur on its two paths, selected as
    tests/test_gpu_lens_blur.py selects them (RTDD_OPT_DEFOCUS_PATH, read back from RTDD_OPT_DEFOCUS_LAST_PATH)."""
    rows, cols = shape
    orig, depth = _rgb(rows, cols, 17), _depth01(rows, cols, 19)
    # the reference's window scale is K = (int)(0.025 * diagonal): 1 .. 6 at these sizes, so defocus sees depths above 255 too (windows of
    # a few pixels: k = K d / 255); refocus and the lens blur take an aperture that gives K = 20 and stay inside [0, 255]
    far = depth.copy()
    far[::2, 1::2] *= np.float32(8.0)
    art = {"artistic": _zeros_like(orig)}
    want = oracle.defocus(orig, far)
    assert (want != orig).any() or rows * cols <= 7
    assert _sweep(ctx, f"defocus path {path} {shape}", {"original": orig, "depth": far}, art,
                  _with_path(ctx, path, lambda im: ctx.GPUSimulateDefocus(im["original"], im["depth"], im["artistic"], rows, cols)), {"artistic": want}) == 49
    aperture = 20.5 / float(np.sqrt(np.float32(rows * rows + cols * cols)))
    _sweep(ctx, f"refocus path {path} {shape}", {"original": orig, "depth": depth}, art,
           _with_path(ctx, path, lambda im: ctx.simulate_refocus(im["original"], im["depth"], im["artistic"], rows, cols, aperture, 100.0, -1, -1)),
           {"artistic": refocus_by_summed_area_table(orig, depth, 100.0, aperture)})
    fx, fy = cols // 2, rows - 1                                     # the pixel form: the focus is read from the view on the device
    _sweep(ctx, f"lens blur path {path} {shape}", {"original": orig, "depth": depth}, art,
           _with_path(ctx, path, lambda im: ctx.simulate_lens_blur(im["original"], im["depth"], im["artistic"], rows, cols, aperture, 0.0, fx, fy, rt.APERTURE_DISC)),
           {"artistic": lens_blur_by_row_prefixes(orig, depth, float(depth[fy, fx]), aperture)})


def _wild_depth(rows, cols, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    d[rng.random((rows, cols)) < 0.03] = np.nan
    return d


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stereo(ctx, shape):
    rows, cols = shape
    orig, depth = _rgb(rows, cols, 21), _wild_depth(rows, cols, 22)
    for mode, D in ((rt.STEREO_VIEW, 5), (rt.STEREO_ANAGLYPH, -7)):
        assert _sweep(ctx, f"stereo mode {mode} {shape}", {"original": orig, "depth": depth}, {"artistic": _zeros_like(orig)},
                      lambda im: ctx.simulate_stereo(im["original"], im["depth"], im["artistic"], rows, cols, D, 100.0, -1, -1, mode),
                      {"artistic": stereo(orig, depth, D, 100.0, mode=mode)}) == 49


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_relight(ctx, shape):
    rows, cols = shape
    orig, depth = _rgb(rows, cols, 23), _wild_depth(rows, cols, 24)
    lights = [light(DIRECTIONAL, -1.0, 0.5, 1.0, relief=0.5, ambient=0.125, diffuse=1.5),
              light(POINT, cols / 3.0, -2.0, 30.0, anchorX=cols // 2, anchorY=rows // 2, radius=40.0, relief=0.25, ambient=0.25, diffuse=2.0, color=(255, 200, 150))]
    for L in lights:
        assert _sweep(ctx, f"relight kind {L['kind']} {shape}", {"original": orig, "depth": depth}, {"artistic": _zeros_like(orig)},
                      lambda im: ctx.simulate_relight(im["original"], im["depth"], im["artistic"], rows, cols, rt.Light(**L)),
                      {"artistic": relight(orig, depth, L)}) == 49
    L, S = lights[0], shadow(8, bias=0.5, softness=0.75, strength=0.875)
    _sweep(ctx, f"relight_shadowed {shape}", {"original": orig, "depth": depth}, {"artistic": _zeros_like(orig)},
           lambda im: ctx.simulate_relight_shadowed(im["original"], im["depth"], im["artistic"], rows, cols, rt.Light(**L), rt.Shadow(**S)),
           {"artistic": relight_shadowed(orig, depth, L, S)})


# ---- cascade pieces -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bgr2gray_pyrdown_gray_depth_to_u8(ctx, oracle, shape):
    rows, cols = shape
    bgr = _rgb(rows, cols, 25)
    assert _sweep(ctx, f"bgr2gray {shape}", {"bgr": bgr}, {"gray": np.zeros(shape, np.uint8)},
                  lambda im: ctx.bgr2gray(im["bgr"], im["gray"], rows, cols), {"gray": oracle.bgr2gray(bgr)}) == 49
    for srows, scols in ((2 * rows - 1, 2 * cols), (2 * rows, 2 * cols - 1)):            # the shape is the destination's: ceil(source / 2)
        src = _u8(srows, scols, 26)
        _sweep(ctx, f"pyrdown_gray {srows}x{scols}", {"src": src}, {"dst": np.zeros(shape, np.uint8)},
               lambda im: ctx.pyrdown_gray(im["src"], srows, scols, im["dst"]), {"dst": oracle.pyrdown_u8(src)})
    depth = np.random.default_rng(27).uniform(-3, 258, shape).astype(np.float32)
    depth[::2, ::2] = np.floor(depth[::2, ::2]) + np.float32(0.5)                         # ties: round half to even
    _sweep(ctx, f"depth_to_u8 {shape}", {"src": depth}, {"dst": np.zeros(shape, np.uint8)},
           lambda im: ctx.depth_to_u8(im["src"], im["dst"], rows, cols), {"dst": oracle.depth_to_u8(depth)})


@pytest.mark.parametrize("shape", SHAPES + [(9, 66), (5, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyrup_depth(ctx, oracle, shape):
    """The shape is the SOURCE's.  Exactly twice the size is cv::cuda::pyrUp (four pixels per thread where the destination's rows allow it:
    (2, 2), (9, 66), (5, 130)); one more row and column is the host's cv::pyrUp with the explicit size."""
    rows, cols = shape
    src = _depth01(rows, cols, 29)
    ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    for drows, dcols in ((2 * rows, 2 * cols), (2 * rows + 1, 2 * cols + 1)):
        assert _sweep(ctx, f"pyrup_depth {shape} -> {drows}x{dcols}", {"src": src}, {"dst": np.zeros((drows, dcols), np.float32)},
                      lambda im: ctx.pyrup_depth(im["src"], rows, cols, im["dst"], drows, dcols), {"dst": oracle.pyrup_f32(src, drows, dcols, contract=1)}) == 49


# ---- copies ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upload_and_download_with_the_device_side_a_view(ctx, shape):
    rows, cols = shape
    L = rt.lib()
    for host in (_rgb(rows, cols, 31), _u8(rows, cols, 32), _depth01(rows, cols, 33)):
        w = host.size // rows * host.itemsize
        for k, (lead, pitch) in enumerate(_layouts(host)):
            dev = Roi(np.zeros_like(host), lead, pitch, FILL_OUTPUT, seed=k, what=f"upload target (lead {lead}, pitch {pitch})")
            ctx._check(L.rtdd_upload(ctx._h, C.c_void_p(dev.ptr), C.c_size_t(pitch), C.c_void_p(host.ctypes.data), C.c_size_t(w), C.c_size_t(w), C.c_int(rows)))
            assert _bits_equal(dev.result(), host)
            src = Roi(host, lead, pitch, FILL_INPUT, what=f"download source (lead {lead}, pitch {pitch})")
            back = np.full((rows, w + 5), 0xA5, np.uint8)                                   # a padded host image: its padding stays too
            ctx._check(L.rtdd_download(ctx._h, C.c_void_p(back.ctypes.data), C.c_size_t(w + 5), C.c_void_p(src.ptr), C.c_size_t(pitch), C.c_size_t(w), C.c_int(rows)))
            assert np.array_equal(back[:, :w], host.reshape(rows, -1).view(np.uint8)) and (back[:, w:] == 0xA5).all()
            tight = np.zeros((rows, w), np.uint8)
            ctx._check(L.rtdd_download(ctx._h, C.c_void_p(tight.ctypes.data), C.c_size_t(w), C.c_void_p(src.ptr), C.c_size_t(pitch), C.c_size_t(w), C.c_int(rows)))
            assert np.array_equal(tight, host.reshape(rows, -1).view(np.uint8))
            src.assert_unchanged()


def test_pyramid_set_image_and_annotation_from_views(oracle, lut):
    """rtdd_pyramid_set_image and _set_annotation read the caller's views; the estimate behind them is the restated cascade's."""
    rows, cols = 37, 70
    bgr = _rgb(rows, cols, 41)
    ann = np.full((rows, cols), 32, np.uint8)
    rng = np.random.default_rng(42)
    for _ in range(6):
        y, x = int(rng.integers(0, rows - 3)), int(rng.integers(0, cols - 5))
        ann[y:y + 3, x:x + 5] = int(rng.choice([0, 64, 128, 192, 254]))
    ref = Cascade(oracle, bgr, ann, lut, 1)
    ref.estimate(20)
    images = [Roi(bgr, l, p, what=f"image (lead {l}, pitch {p})") for l, p in _layouts(bgr)]
    anns = [Roi(ann, l, p, what=f"annotation (lead {l}, pitch {p})") for l, p in _layouts(ann)]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == ref.P
        for i, a in itertools.product(images, anns):
            c.pyramid_set_image(i.img); c.pyramid_set_annotation(a.img)
            c.estimate_depth(20); c.synchronize()
            what = f"{i.what}, {a.what}"
            assert np.array_equal(c.pyramid_download(rt.IMG_ORIGINAL), bgr), what
            assert np.array_equal(c.pyramid_download(rt.IMG_GRAY), ref.gray[0]), what
            assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE), ref.scribble[0]) and np.array_equal(c.pyramid_download(rt.IMG_EDITED), ref.edited[0]), what
            assert _bits_equal(c.pyramid_download(rt.IMG_DEPTH), ref.depth[0]), what
            assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), ref.depth_u8), what
            i.assert_unchanged(); a.assert_unchanged()


# ---- the f32 alignment contract -------------------------------------------------------------------------------------------------------------
def test_f32_alignment_is_refused(ctx):
    """Every entry point that takes an f32 image returns RTDD_ERR_INVALID (1), with a message, for a pitch of cols * 4 + 2 and, separately,
    for a pointer of base + 2; nothing is launched (the pre-filled outputs keep every byte); the same context then serves the legal call.
    u8 images stay legal at any pointer and pitch (every other test of this file)."""
    rows, cols = 9, 67
    depth, mask, gray = _problem(rows, cols, 51)
    orig = _rgb(rows, cols, 52)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    import torch
    idx = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda:0")
    L, S = light(DIRECTIONAL, 0, 0, 1), shadow(8)
    o, g, m = Roi(orig, 1, what="original"), Roi(gray, 3, what="gray"), Roi(mask, 2, what="scribble")
    small = Roi(_depth01(4, 33, 53), 4, what="pyrUp source")

    def effect(fn, *extra):
        return lambda d, out: fn(o.img, d, out.img, rows, cols, *extra)
    # name -> (the call with its f32 image `d` and its u8 or second image `out`, the host image `out` starts from)
    art = np.zeros_like(orig)
    entries = {
        "rtdd_matrix_free_solver": (lambda d, out: ctx.GPUMatrixFreeSolver(d, m.img, g.img, rows, cols, 0.4, 9, 0.0, 0), None),
        "rtdd_solve_ex": (lambda d, out: ctx.solve_ex(d, m.img, g.img, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=3), None),
        "rtdd_index_to_weight": (lambda d, out: ctx.index_to_weight(g.img, d, idx, 0, rows, cols), None),
        "rtdd_convert_to_float": (lambda d, out: ctx.GPUConvertToFloat(o.img, d, m.img, rows, cols), None),
        "rtdd_depth_to_u8": (lambda d, out: ctx.depth_to_u8(d, out.img, rows, cols), np.zeros((rows, cols), np.uint8)),
        "rtdd_pyrup_depth (destination)": (lambda d, out: ctx.pyrup_depth(small.img, 4, 33, d, rows, cols), None),
        "rtdd_pyrup_depth (source)": (lambda d, out: ctx.pyrup_depth(d, rows, cols, out.img, 2 * rows, 2 * cols), np.zeros((2 * rows, 2 * cols), np.float32)),
        "rtdd_simulate_defocus": (effect(ctx.GPUSimulateDefocus), art),
        "rtdd_simulate_desaturation": (lambda d, out: ctx.GPUSimulateDesaturation(o.img, g.img, d, out.img, rows, cols), art),
        "rtdd_simulate_haze": (effect(ctx.GPUSimulateHaze), art),
        "rtdd_simulate_haze_ex": (effect(ctx.simulate_haze_ex, 1.5, (255, 255, 255)), art),
        "rtdd_simulate_refocus": (effect(ctx.simulate_refocus, 0.025, 100.0, -1, -1), art),
        "rtdd_simulate_lens_blur (disc)": (effect(ctx.simulate_lens_blur, 0.025, 100.0, -1, -1, rt.APERTURE_DISC), art),
        "rtdd_simulate_lens_blur (box)": (effect(ctx.simulate_lens_blur, 0.025, 100.0, -1, -1, rt.APERTURE_BOX), art),
        "rtdd_simulate_stereo": (effect(ctx.simulate_stereo, 5, 100.0, -1, -1, rt.STEREO_VIEW), art),
        "rtdd_simulate_relight": (effect(ctx.simulate_relight, rt.Light(**L)), art),
        "rtdd_simulate_relight_shadowed": (effect(ctx.simulate_relight_shadowed, rt.Light(**L), rt.Shadow(**S)), art),
    }
    pitch = pitch_for(cols * 4, 0, 0)
    for name, (call, out_host) in entries.items():
        for form in ("pitch", "pointer"):
            d = Roi(depth, 0, pitch, FILL_OUTPUT, seed=3, what=f"{name}: the f32 image")
            out = Roi(out_host, 4 if out_host.dtype == np.float32 else 2, None, FILL_OUTPUT, seed=4, what=f"{name}: the output") if out_host is not None else None
            bad = (d.ptr, cols * 4 + 2) if form == "pitch" else (d.ptr + 2, pitch)
            with pytest.raises(rt.RtddError) as e:
                call(bad, out)
            ctx.synchronize()
            assert e.value.status == 1 and "multiples of 4" in str(e.value), (name, form, str(e.value))
            assert _bits_equal(d.result(), depth), (name, form)                              # (result() checks every byte around the view)
            if out is not None:
                assert _bits_equal(out.result(), out_host), (name, form)
        d = Roi(depth, 4, pitch + 4, FILL_OUTPUT, seed=5, what=f"{name}: the f32 image, legal")
        out = Roi(out_host, 4 if out_host.dtype == np.float32 else 2, None, FILL_OUTPUT, seed=6, what=f"{name}: the output") if out_host is not None else None
        call(d.img, out)                                                                     # the same context still serves a legal call
        ctx.synchronize()
        d.result()
        if out is not None:
            assert not _bits_equal(out.result(), out_host), name                             # (something was launched this time)
    for r in (o, g, m, small):
        r.assert_unchanged()
