"""The depth regions on the GPU (-m gpu): rtdd_index_to_weight_regions, rtdd_solve_regions, rtdd_region_codes and the pyramid's regions
(rtdd_pyramid_set_regions, the paint calls on the region pair) against the restatement of tests/regions_ref.py, bit for bit.

Shapes of the index pass and the solve: the colour guide's -- 1x1, 1x7, 9x1, 5x67, 33x130, 6x256, 6x257, 6x260, 7x515: ragged groups of
four pixels and both sides of the 256-pixel span of one workgroup's four-pixel threads.  Levels: (2 of 2) un-gated, (1 of 2) gated with
threshold 4, (0 of 2) gated with threshold 0.  Both guides, all three flag values.  Code images: a pattern of pairs under random
rectangles of ids (0 included), a one-pixel region, a one-pixel-wide line, a two-id checkerboard band in which every edge is cut (and a
pixel inside it has a denormal divisor).  Estimates: 181 x 243 (three levels), maxIterations 64, the regions painted through
rtdd_fill_polygon and rtdd_fill_similar on the pyramid's own region pair.  Every comparison of two GPU results is accompanied by a
comparison of one of them with the CPU restatement."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import np_restatement as npr
import polygon_ref as pr
import realtimedepthdiffusion_amd as rt
import regions_ref as rr
import wand_ref as wr
from cascade_ref import Cascade
from color_guide_ref import BGR, GRAY
from effect_gpu import harness_bin, harness_files, run_harness, write_pnm
from gpu_util import assert_bit_equal, down, up
from roi_util import FILL_OUTPUT, Roi, pitch_for

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 7), (9, 1), (5, 67), (33, 130), (6, 256), (6, 257), (6, 260), (7, 515)]
SHAPE_IDS = [f"{r}x{c}" for r, c in SHAPES]
REGIMES = [(2, 2), (1, 2), (0, 2)]              # (level, maxLevel)
ALL_FLAGS = [rr.CUT, rr.SMOOTH, rr.CUT | rr.SMOOTH]
BOTH = rr.CUT | rr.SMOOTH
ROWS, COLS, ITERS = 181, 243, 64                # the estimates


@pytest.fixture(scope="module")
def ctx():
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        yield c


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _guide(kind, rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3) if kind == BGR else (rows, cols), dtype=np.uint8)


def _depth(rows, cols, seed):
    """u8 values 100 + cx[x % 7] + cy[y % 6] under a fraction in [0, 0.9): neighbouring differences on both sides of both thresholds."""
    cx = np.array([0, 0, 3, 9, 9, 4, 10]); cy = np.array([0, 0, 2, 8, 8, 1])
    d = 100 + cx[np.arange(cols) % 7][None, :] + cy[np.arange(rows) % 6][:, None]
    return (d + np.random.default_rng(seed).uniform(0, 0.9, (rows, cols))).astype(np.float32)


def _mask(rows, cols, seed):
    m = np.where(np.random.default_rng(seed).random((rows, cols)) < 0.12, 255, 32).astype(np.uint8)
    m[rows // 2, cols // 2] = 255
    return m


def _problem(rows, cols, seed, kind):
    depth, mask = _depth(rows, cols, seed), _mask(rows, cols, seed + 1)
    lab = np.random.default_rng(seed + 2).integers(0, 256, (rows, cols)).astype(np.float32)
    depth[mask == 255] = lab[mask == 255]
    return depth, mask, _guide(kind, rows, cols, seed + 3)


CODE_KINDS = ["rects", "pixel", "line", "checker"]


def _codes(rows, cols, kind, seed=0):
    yy, xx = np.mgrid[:rows, :cols]
    if kind == "pixel":                                     # a one-pixel region
        c = np.zeros((rows, cols), np.uint8); c[rows // 2, cols // 2] = 5
    elif kind == "line":                                    # a one-pixel-wide line, across a row and down a column
        c = np.zeros((rows, cols), np.uint8); c[rows // 2, :] = 9; c[:, cols // 3] = 9
    elif kind == "checker":                                 # a band of two ids in which every edge is cut, unassigned pixels around it
        c = np.where((yy >= rows // 4) & (yy <= rows - 1 - rows // 4), 1 + (yy + xx) % 2, 0).astype(np.uint8)
    else:
        # pairs of pixels 0 0 | 7 7 | 0 0 | 200 200 along both axes: an untouched, a cut and a smoothed edge within any five pixels ...
        c = np.array([0, 7, 0, 200], np.uint8)[(xx // 2 + yy // 2) % 4]
        if rows >= 5 and cols >= 60:                        # ... under random rectangles of ids, 0 included, right of the first 16 columns
            rng = np.random.default_rng(seed + rows * 1000 + cols)
            for _ in range(6):
                y0, x0 = int(rng.integers(0, rows)), int(rng.integers(16, cols))
                c[y0:y0 + int(rng.integers(1, rows + 1)), x0:x0 + int(rng.integers(1, cols // 2))] = rng.choice([0, 1, 2, 255])
    return np.ascontiguousarray(c)


def _assert_every_kind_of_edge(codes):
    """(on the CPU) some edge is cut, some smoothed and some left alone -- for every shape that has an edge"""
    c = codes.astype(np.int32)
    pairs = np.concatenate([np.stack([c[:, 1:].ravel(), c[:, :-1].ravel()]), np.stack([c[1:].ravel(), c[:-1].ravel()])], axis=1)
    if codes.size == 1:
        assert pairs.shape[1] == 0
        return
    a, b = pairs
    assert (a != b).any() and ((a == b) & (a != 0)).any() and ((a == 0) & (b == 0)).any()


def _allocate(c, rows, cols, level, max_level):
    c.GPUAllocateDeviceMemory(rows << level, cols << level, max_level + 1)


# ---- 1. the index pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_index_pass_matches_the_restatement(ctx, shape):
    rows, cols = shape
    depth = _depth(rows, cols, 20 + cols)
    d = up(depth)
    _assert_every_kind_of_edge(_codes(rows, cols, "rects"))
    cases = [("rects", f) for f in ALL_FLAGS] + [(k, BOTH) for k in CODE_KINDS[1:]]
    for kind in (GRAY, BGR):
        guide = _guide(kind, rows, cols, 10 + cols + kind)
        g = up(guide)
        for level, max_level in REGIMES:
            _allocate(ctx, rows, cols, level, max_level)
            base = rr.base_maps(guide, kind, depth, level, max_level)
            for code_kind, flags in cases:
                codes = _codes(rows, cols, code_kind)
                out = torch.full((rows, cols, 2), -1, dtype=torch.int32, device="cuda:0")
                ctx.index_to_weight_regions(g, kind, up(codes), flags, d, out, level, rows, cols)
                ctx.synchronize()
                want = npr.pack_index(rr.index_maps_regions(base, codes, flags))
                assert np.array_equal(out.cpu().numpy(), want), f"{rows}x{cols} guide {kind} level {level} of {max_level} codes {code_kind} flags {flags}"
            # no regions, flags 0 and all-zero codes: the guided pass
            for regions, flags in ((None, 0), (up(_codes(rows, cols, "rects")), 0), (up(np.zeros((rows, cols), np.uint8)), BOTH)):
                out = torch.full((rows, cols, 2), -1, dtype=torch.int32, device="cuda:0")
                ctx.index_to_weight_regions(g, kind, regions, flags, d, out, level, rows, cols)
                ctx.synchronize()
                assert np.array_equal(out.cpu().numpy(), npr.pack_index(base))


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_region_solve_matches_the_restatement(ctx, lut, shape):
    rows, cols = shape
    iters = 24
    try:
        for kind in (GRAY, BGR):
            depth, mask, guide = _problem(rows, cols, 40 + cols + kind, kind)
            m, g = up(mask), up(guide)
            for level, max_level in REGIMES:
                _allocate(ctx, rows, cols, level, max_level)
                cases = [("rects", f) for f in ALL_FLAGS]
                if kind == GRAY and level == 0:
                    cases += [(k, BOTH) for k in CODE_KINDS[1:]]
                for code_kind, flags in cases:
                    codes = _codes(rows, cols, code_kind)
                    r = up(codes)
                    want = rr.solve_regions(depth, mask, guide, kind, codes, flags, iters, level, max_level, lut, 1)
                    for kernel in (1, 2):
                        ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel)
                        d = up(depth)
                        assert ctx.solve_regions(d, m, g, kind, r, flags, rows, cols, level, maxIterations=iters)[0] == iters
                        ctx.synchronize()
                        assert ctx.last_solve_info().kernel == kernel
                        assert_bit_equal(down(d), want, f"{rows}x{cols} guide {kind} level {level} of {max_level} codes {code_kind} flags {flags} kernel {kernel}")
        # without FP contraction, once
        depth, mask, guide = _problem(rows, cols, 60 + cols, GRAY)
        codes = _codes(rows, cols, "rects")
        _allocate(ctx, rows, cols, 0, 0)
        ctx.set_option(rt.OPT_FP_CONTRACT, 0); ctx.set_option(rt.OPT_SWEEP_KERNEL, 0)
        d = up(depth)
        ctx.solve_regions(d, up(mask), up(guide), GRAY, up(codes), BOTH, rows, cols, 0, maxIterations=iters)
        ctx.synchronize()
        assert_bit_equal(down(d), rr.solve_regions(depth, mask, guide, GRAY, codes, BOTH, iters, 0, 0, lut, 0), f"{rows}x{cols} without contraction")
    finally:
        ctx.set_option(rt.OPT_SWEEP_KERNEL, 0); ctx.set_option(rt.OPT_FP_CONTRACT, 1)


# ---- 3. both forms of the prepare kernels: aligned codes and a region of interest; stray writes ----------------------------------------------
# (lead bytes, pitch residue) of the code image: aligned (the four-pixel kernel), pointers off by 1..3 bytes, odd pitches (the scalar one)
CODE_LAYOUTS = [(0, 0), (1, 0), (2, 4), (3, 1), (0, 3), (1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_aligned_codes_and_region_of_interest_give_the_same_bits(ctx, lut, shape):
    rows, cols = shape
    for kind in (GRAY, BGR):
        depth, mask, guide = _problem(rows, cols, 70 + cols + kind, kind)
        codes = _codes(rows, cols, "rects", seed=1)
        m, g = up(mask), up(guide)
        for level, max_level in ((0, 0), (1, 2)):               # un-gated, and gated: the row below is read for the depth gate too
            _allocate(ctx, rows, cols, level, max_level)
            want = rr.solve_regions(depth, mask, guide, kind, codes, BOTH, 8, level, max_level, lut, 1)
            results = []
            for lead, residue in CODE_LAYOUTS:
                roi = Roi(codes, lead, pitch_for(cols, lead, residue), what=f"codes (lead {lead}, residue {residue})")
                assert (roi.ptr % 4 == 0 and roi.pitch % 4 == 0) == ((lead, residue) == (0, 0))
                d = Roi(depth, 0, pitch_for(cols * 4, 0, 0), fill=FILL_OUTPUT, seed=lead, what="depth")
                ctx.solve_regions(d.img, m, g, kind, roi.img, BOTH, rows, cols, level, maxIterations=8)
                ctx.synchronize()
                roi.assert_unchanged()                          # (0xFF all around the view: a byte read from there would change an index)
                results.append(d.result())                      # (nothing written around the depth map)
            for (lead, residue), got in zip(CODE_LAYOUTS, results):
                assert_bit_equal(got, results[0], f"{rows}x{cols} guide {kind} level {level}: lead {lead}, residue {residue} against the aligned codes")
            assert_bit_equal(results[0], want, f"{rows}x{cols} guide {kind} level {level}: the aligned codes against the restatement")


# ---- 4. no regions is rtdd_solve_guided --------------------------------------------------------------------------------------------------------
def test_null_regions_or_flags_0_is_solve_guided(ctx, lut):
    rows, cols = 33, 130
    depth, mask, gray = _problem(rows, cols, 120, GRAY)
    codes = _codes(rows, cols, "rects")
    _allocate(ctx, rows, cols, 0, 0)
    m, g, r = up(mask), up(gray), up(codes)
    a, b, c0, z = up(depth), up(depth), up(depth), up(depth)
    ctx.solve_guided(a, m, g, GRAY, rows, cols, 0, maxIterations=40); info_a = ctx.last_solve_info()
    ctx.solve_regions(b, m, g, GRAY, None, 0, rows, cols, 0, maxIterations=40); info_b = ctx.last_solve_info()
    ctx.solve_regions(c0, m, g, GRAY, r, 0, rows, cols, 0, maxIterations=40); info_c = ctx.last_solve_info()
    ctx.solve_regions(z, m, g, GRAY, up(np.zeros_like(codes)), BOTH, rows, cols, 0, maxIterations=40)
    ctx.synchronize()
    assert info_a.describe() == info_b.describe() == info_c.describe()
    assert_bit_equal(down(a), npr.solve(depth, mask, gray, 40, 0, 0, lut, 1), "rtdd_solve_guided against the restatement")
    assert_bit_equal(down(b), down(a), "null regions against rtdd_solve_guided")
    assert_bit_equal(down(c0), down(a), "flags 0 against rtdd_solve_guided")
    assert_bit_equal(down(z), down(a), "all-zero codes against rtdd_solve_guided")


# ---- 5. the other methods read the same indices ------------------------------------------------------------------------------------------
def test_blocked_persistent_and_red_black_with_regions(ctx, oracle, lut):
    rows, cols = 33, 130
    depth, mask, gray = _problem(rows, cols, 130, GRAY)
    codes = _codes(rows, cols, "rects")
    _allocate(ctx, rows, cols, 0, 0)
    m, g, r = up(mask), up(gray), up(codes)
    maps = rr.index_maps_regions(npr.index_maps(gray, depth, 0, 0), codes, BOTH)
    d = up(depth)
    ctx.solve_regions(d, m, g, GRAY, r, BOTH, rows, cols, 0, maxIterations=40)          # the automatic choice: the blocked kernel, persistent
    info = ctx.last_solve_info()
    ctx.synchronize()
    assert info.kernel == 2, info.describe()
    print("blocked solve with regions:", info.describe())
    assert_bit_equal(down(d), rr.solve_maps(depth, mask, maps, 40, lut, 1), "blocked / persistent")
    want = depth.copy()
    idx = np.ascontiguousarray(npr.pack_index(maps))
    for _ in range(9):
        oracle.rbgs_sweep(want, idx, mask, lut, 1)
    try:
        for kernel in (0, 1):
            ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel)
            d = up(depth)
            ctx.solve_regions(d, m, g, GRAY, r, BOTH, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=9)
            ctx.synchronize()
            assert_bit_equal(down(d), want, f"red-black, sweep kernel option {kernel}")
    finally:
        ctx.set_option(rt.OPT_SWEEP_KERNEL, 0)


# ---- 6. rtdd_region_codes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,levels", [(181, 243, 3), (1, 1, 1)])
def test_region_codes_match_the_restatement(ctx, rows, cols, levels):
    rng = np.random.default_rng(rows)
    edited = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    mask = np.where(rng.random((rows, cols)) < 0.6, 255, rng.integers(0, 255, (rows, cols))).astype(np.uint8)
    e, m = Roi(edited, 1, pitch_for(cols * 3, 1, 3), what="region edited"), Roi(mask, 3, pitch_for(cols, 3, 1), what="region mask")
    for level in range(levels):
        want = rr.region_codes(edited, mask, level)
        out = Roi(np.zeros_like(want), 1, pitch_for(want.shape[1], 1, 2), fill=FILL_OUTPUT, seed=level, what=f"codes of level {level}")
        ctx.region_codes(e.img, m.img, rows, cols, level, out.img)
        ctx.synchronize()
        assert np.array_equal(out.result(), want), f"level {level}"
    e.assert_unchanged(); m.assert_unchanged()
    # a level too coarse to hold a pixel writes nothing
    out = Roi(np.zeros((1, 1), np.uint8), 0, fill=FILL_OUTPUT, what="codes of an empty level")
    ctx.region_codes(e.img, m.img, rows, cols, 8, out.img)
    ctx.synchronize()
    assert np.array_equal(out.parent(), out.filled)


# ---- 7. the estimate -----------------------------------------------------------------------------------------------------------------------
POLYGON = [(30, 20), (120, 25), (110, 90), (40, 100)]       # region 1: a lasso
WAND = wr.constant(200, 150, 60, 2)                         # region 2: a click, tolerance 60 on the photograph


def _blocks(seed, rows=ROWS, cols=COLS, block=16):
    """A random colour per 16 x 16 block."""
    small = np.random.default_rng(seed).integers(0, 256, (-(-rows // block), -(-cols // block), 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, block, 0), block, 1)[:rows, :cols])


def _annotation(rows=ROWS, cols=COLS, shift=0):
    """Three labels: 0, 128 and 254."""
    ann = np.full((rows, cols), 32, np.uint8)
    ann[rows // 8: rows // 8 + 6, cols // 8 + shift: cols // 2] = 0
    ann[rows // 2: rows // 2 + 5, cols // 2: cols - 12 - shift] = 128
    ann[rows - 20: rows - 15, 10 + shift: cols // 3] = 254
    return ann


def _paint_ref(ref, bgr, shift=0, first_id=1):
    poly = [(x + shift, y) for x, y in POLYGON]
    assert pr.fill_polygon(poly, pr.constant(first_id), ref.region_edited, ref.region_mask, bgr) > 1000
    wand = WAND[:8] + (first_id + 1, first_id + 1)
    assert wr.fill_similar(wand, ref.region_edited, ref.region_mask, bgr, wr.covered_label)[0] >= 256
    return ref


def _paint_gpu(c, rows=ROWS, cols=COLS, shift=0, first_id=1):
    """the same two regions through rtdd_fill_polygon and rtdd_fill_similar on the pyramid's own region pair"""
    e, m, o = c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], c.pyramid_image(rt.IMG_ORIGINAL)[:2]
    c.fill_polygon([(x + shift, y) for x, y in POLYGON], pr.constant(first_id), e, m, rows, cols)
    return c.fill_similar(WAND[:8] + (first_id + 1, first_id + 1), e, m, rows, cols, o)


@pytest.fixture(scope="module")
def refs(oracle, lut):
    """The CPU references the estimate tests share, computed once and left as they are."""
    t = min(8, oracle.max_threads())
    out = {"bgr": _blocks(1), "ann": _annotation()}
    for name, guide in (("gray", GRAY), ("colour", BGR)):
        out[name] = _paint_ref(rr.RegionCascade(oracle, out["bgr"], out["ann"], lut, 1, t, guide=guide, flags=BOTH), out["bgr"])
        out[name].estimate(ITERS)
    out["plain"] = Cascade(oracle, out["bgr"], out["ann"], lut, 1, t); out["plain"].estimate(ITERS)
    # flags 0 for one estimate, then both flags for the next, which continues from the first one's depth pyramid
    tg = _paint_ref(rr.RegionCascade(oracle, out["bgr"], out["ann"], lut, 1, t, guide=GRAY, flags=0), out["bgr"])
    tg.estimate(ITERS)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(tg.depth, out["plain"].depth))
    tg.flags = BOTH; tg.estimate(ITERS)
    out["toggled"] = tg
    codes = out["gray"].codes(0)
    assert set(np.unique(codes)) == {0, 1, 2}
    assert not np.array_equal(out["gray"].depth_u8, out["plain"].depth_u8) and not np.array_equal(out["gray"].depth_u8, out["colour"].depth_u8)
    return out


def _setup(c, bgr, ann, guide, flags, create=True, **paint):
    if create:
        c.pyramid_create(bgr.shape[0], bgr.shape[1])
    c.pyramid_set_guide(guide)
    c.pyramid_set_regions(BOTH)
    c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
    info = _paint_gpu(c, bgr.shape[0], bgr.shape[1], **paint)
    c.pyramid_set_regions(flags)
    assert c.pyramid_regions() == flags
    return info


def _assert_levels(c, ref, what):
    for l in range(ref.P - 1, -1, -1):
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), ref.depth[l], f"{what}: depth level {l}")
    assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), ref.depth_u8), f"{what}: u8 map"


@pytest.mark.parametrize("name,guide", [("gray", rt.GUIDE_GRAY), ("colour", rt.GUIDE_BGR)])
def test_estimate_with_regions(ctx, refs, name, guide):
    ref = refs[name]
    info = _setup(ctx, refs["bgr"], refs["ann"], guide, BOTH)
    assert info.pixels == int((ref.codes(0) == 2).sum())
    ctx.estimate_depth(ITERS); ctx.synchronize()
    assert ref.P == 3
    _assert_levels(ctx, ref, f"{name} guide, cut and smooth")
    assert np.array_equal(ctx.pyramid_download(rt.IMG_REGION_EDITED), ref.region_edited)
    assert np.array_equal(ctx.pyramid_download(rt.IMG_REGION_MASK), ref.region_mask)
    for l in range(ref.P):
        got = ctx.pyramid_download(rt.IMG_REGION_CODE, l)
        assert got.shape == ref.size[l] and np.array_equal(got, ref.codes(l)), f"codes of level {l}"


def test_toggling_the_flags(refs):
    """Flags 0 with the region images kept: the plain estimate's bits; both flags again: the next estimate applies them, from the first
    one's depth pyramid.  rtdd_refine_depth follows the flags."""
    ref = refs["toggled"]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _setup(c, refs["bgr"], refs["ann"], rt.GUIDE_GRAY, 0)
        c.estimate_depth(ITERS); c.synchronize()
        _assert_levels(c, refs["plain"], "flags 0 against the estimate of a pyramid without regions")
        assert not c.pyramid_download(rt.IMG_REGION_CODE, 0).any()      # (nothing was launched for them)
        c.pyramid_set_regions(BOTH)
        c.estimate_depth(ITERS); c.synchronize()
        _assert_levels(c, ref, "both flags, behind the plain estimate")
        assert np.array_equal(c.pyramid_download(rt.IMG_REGION_CODE, 1), ref.codes(1))
        c.refine_depth(method=rt.METHOD_CHEBYSHEV_JACOBI, maxIterations=5, tolerance=0.0)
        c.synchronize()
        want = rr.solve_regions(ref.depth[0], ref.scribble[0], ref.gray[0], GRAY, ref.codes(0), BOTH, 5, 0, ref.P - 1, ref.lut, 1)
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, 0), want, "refine with regions")


def _upload(c, host, ptr, pitch):
    host = np.ascontiguousarray(host)
    width = host.size // host.shape[0] * host.itemsize
    c._check(rt.lib().rtdd_upload(c._h, C.c_void_p(ptr), C.c_size_t(pitch), C.c_void_p(host.ctypes.data), C.c_size_t(width), C.c_size_t(width), C.c_int(host.shape[0])))


def test_a_region_paint_leaves_the_annotation_and_its_state_alone(oracle, lut):
    """91 x 123, two levels.  After an estimate the coarse annotation level is up to date.  A foreign write (another context's upload,
    behind this one's back) then adds one label to the level-0 annotation and removes another.  Every paint call on the REGION pair, an
    erasing one included, must leave that unnoticed: the next estimate does not touch the coarse level.  rtdd_pyramid_annotation_changed
    then brings the added label in and -- the coarse levels only ever accumulate, and no rebuild was asked for -- keeps the removed one."""
    rows, cols, iters = 91, 123, 8
    bgr, ann = _blocks(7, rows, cols), _annotation(rows, cols)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == 2
        c.pyramid_set_regions(rr.CUT)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(iters); c.synchronize()
        s0, e0 = c.pyramid_download(rt.IMG_SCRIBBLE, 0), c.pyramid_download(rt.IMG_EDITED, 0)
        s1 = c.pyramid_download(rt.IMG_SCRIBBLE, 1)
        # foreign: a new label in the bottom right corner, the label 0 strip at the top removed
        s0n, e0n = s0.copy(), e0.copy()
        s0n[rows - 12:rows - 4, cols - 30:cols - 6] = 255; e0n[rows - 12:rows - 4, cols - 30:cols - 6] = 77
        gone = (s0 == 255) & (e0[..., 0] == 0)
        assert gone.sum() > 100
        s0n[gone] = 0; e0n[gone] = bgr[gone]
        sp, spitch = c.pyramid_image(rt.IMG_SCRIBBLE)[:2]; ep, epitch = c.pyramid_image(rt.IMG_EDITED)[:2]
        with rt.Context(0) as other:
            _upload(other, s0n, sp, spitch); _upload(other, e0n, ep, epitch)
        # every paint call, on the region pair
        e, m, o = c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], c.pyramid_image(rt.IMG_ORIGINAL)[:2]
        c.GPUPaintImage(20, 20, 3, 9, e, m, rows, cols)
        c.paint_strokes([(5, 40, 60, 44, 5, rt.BRUSH_ROUND, 4), (5, 40, 30, 42, 3, rt.BRUSH_SQUARE, rt.STROKE_ERASE)], e, m, rows, cols, original=o)
        c.paint_ramp_strokes([(70, 10, 110, 30, 4, rt.BRUSH_SQUARE, 5, 9)], e, m, rows, cols)
        c.fill_polygon([(60, 50), (110, 52), (90, 85)], pr.constant(6), e, m, rows, cols)
        c.fill_polygon([(70, 55), (90, 56), (85, 70)], pr.erase(), e, m, rows, cols, original=o)
        c.fill_similar(wr.constant(8, 80, 30, 7), e, m, rows, cols, o)
        c.estimate_depth(iters); c.synchronize()
        assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE, 0), s0n) and np.array_equal(c.pyramid_download(rt.IMG_EDITED, 0), e0n)
        assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE, 1), s1), "a region paint marked the annotation as changed"
        codes = c.pyramid_download(rt.IMG_REGION_CODE, 0)
        assert set(np.unique(codes)) >= {0, 3, 4, 6, 7} and np.array_equal(codes, rr.region_codes(c.pyramid_download(rt.IMG_REGION_EDITED), c.pyramid_download(rt.IMG_REGION_MASK), 0))
        assert np.array_equal(c.pyramid_download(rt.IMG_REGION_CODE, 1), codes[::2, ::2][:rows // 2, :cols // 2])
        c.pyramid_annotation_changed()
        c.estimate_depth(iters); c.synchronize()
        s1n = c.pyramid_download(rt.IMG_SCRIBBLE, 1)
        want = Cascade(oracle, bgr, ann, lut, 1, 1)
        want.estimate(0)
        assert np.array_equal(want.scribble[1], s1)
        want.scribble[0][...] = s0n; want.edited[0][...] = e0n
        want.estimate(0)                                                 # (accumulates into the coarse level it has)
        assert np.array_equal(s1n, want.scribble[1]) and (s1n >= s1).all() and (s1n > s1).any(), "an erasing region paint asked for the annotation rebuild"


# ---- 8. a batch ------------------------------------------------------------------------------------------------------------------------------
def test_batch_with_different_regions_per_image(ctx, refs):
    images = [refs["bgr"], _blocks(2), _blocks(3)]
    anns = [refs["ann"], _annotation(shift=9), _annotation(shift=17)]
    paints = [dict(shift=0, first_id=1), dict(shift=25, first_id=3), dict(shift=60, first_id=200)]
    singles = []
    for bgr, ann, paint in zip(images, anns, paints):
        _setup(ctx, bgr, ann, rt.GUIDE_GRAY, BOTH, **paint)
        ctx.estimate_depth(ITERS); ctx.synchronize()
        singles.append(([ctx.pyramid_download(rt.IMG_DEPTH, l) for l in range(3)], ctx.pyramid_download(rt.IMG_DEPTH_U8),
                        [ctx.pyramid_download(rt.IMG_REGION_CODE, l) for l in range(3)]))
    assert_bit_equal(singles[0][0][0], refs["gray"].depth[0], "the first single-image estimate against the restatement")
    assert not np.array_equal(singles[0][2][0], singles[1][2][0]) and not np.array_equal(singles[1][2][0], singles[2][2][0])
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create_batch(ROWS, COLS, 3) == 3
        for b, (bgr, ann, paint) in enumerate(zip(images, anns, paints)):
            c.pyramid_select(b)
            _setup(c, bgr, ann, rt.GUIDE_GRAY, BOTH, create=False, **paint)
        c.estimate_depth_batch(ITERS); c.synchronize()
        for b in range(3):
            c.pyramid_select(b)
            for l in range(3):
                assert np.array_equal(c.pyramid_download(rt.IMG_REGION_CODE, l), singles[b][2][l]), f"image {b} codes of level {l}"
                assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), singles[b][0][l], f"image {b} level {l}")
            assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), singles[b][1]), f"image {b} u8 map"


# ---- 9. live frames ------------------------------------------------------------------------------------------------------------------------
def test_live_frames_with_regions(refs):
    ref = refs["gray"]
    with rt.Context(0) as c:                                            # what rtdd_estimate_depth gives, frame by frame (warm starts)
        c.GPULoadWeights(0.4)
        _setup(c, refs["bgr"], refs["ann"], rt.GUIDE_GRAY, BOTH)
        c.estimate_depth(ITERS); c.synchronize()
        want = [c.pyramid_download(rt.IMG_DEPTH_U8)]
        c.estimate_depth(ITERS); c.synchronize()
        want.append(c.pyramid_download(rt.IMG_DEPTH_U8))
    assert np.array_equal(want[0], ref.depth_u8)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(ROWS, COLS)
        c.pyramid_set_regions(BOTH)
        c.pyramid_set_image(up(refs["bgr"]))
        _paint_gpu(c)
        c.synchronize()
        scr = rt.host_image((ROWS, COLS)); ed = rt.host_image((ROWS, COLS, 3)); out = [rt.host_image((ROWS, COLS)) for _ in range(2)]
        scr.a[...] = ref.scribble[0]; ed.a[...] = ref.edited[0]
        for n in range(2):
            c.live_submit(scr.a, ed.a, out[n].a, ITERS)
        assert c.live_pending() == 2
        got = []
        for n in range(2):
            c.live_wait(); got.append(out[n].a.copy())
        c.synchronize()
        for n in range(2):
            assert np.array_equal(got[n], want[n]), f"frame {n}"


# ---- 10. a healed time-out replays a region call with its regions ---------------------------------------------------------------------------
def test_healed_solve_and_estimate_keep_their_regions(lut, refs, capfd):
    """(the debug route of the colour guide's heal test: the status word forced behind the next blocked launch, nothing made to wait)"""
    rows, cols = 33, 130
    depth, mask, gray = _problem(rows, cols, 150, GRAY)
    codes = _codes(rows, cols, "rects")
    want = rr.solve_regions(depth, mask, gray, GRAY, codes, BOTH, 24, 0, 0, lut, 1)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.GPUAllocateDeviceMemory(rows, cols, 1)
        d, m, g, r = up(depth), up(mask), up(gray), up(codes)
        c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
        c.solve_regions(d, m, g, GRAY, r, BOTH, rows, cols, 0, maxIterations=24)
        assert c.last_solve_info().kernel == 2
        c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        assert_bit_equal(down(d), want, "healed region solve")
    ref = refs["gray"]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _setup(c, refs["bgr"], refs["ann"], rt.GUIDE_GRAY, BOTH)
        c.synchronize()
        c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
        c.estimate_depth(ITERS)
        c.pyramid_set_regions(0)                                    # the replay must not look here
        c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        assert c.pyramid_regions() == 0
        _assert_levels(c, ref, "healed region estimate, the pyramid's flags switched off before the synchronisation")
    capfd.readouterr()                                                  # (the heal's one warning on stderr)


# ---- 11. refusals, before any launch -------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rows, cols = 9, 21
    depth, mask, gray = _problem(rows, cols, 170, GRAY)
    codes = _codes(rows, cols, "rects")
    _allocate(ctx, rows, cols, 0, 0)
    d, m, g, r = up(depth), up(mask), up(gray), up(codes)
    L = rt.lib()
    params = rt.SolveParams(rt.METHOD_CHEBYSHEV_JACOBI, 5, 0.0, 0, 0.0)

    def solve(region_ptr, region_pitch, flags, guide_kind=GRAY, guide_pitch=None):
        return L.rtdd_solve_regions(ctx._h, C.c_void_p(d.data_ptr()), C.c_size_t(d.stride(0) * 4), C.c_void_p(m.data_ptr()), C.c_size_t(m.stride(0)),
                                    C.c_void_p(g.data_ptr()), C.c_size_t(g.stride(0) if guide_pitch is None else guide_pitch), C.c_int(guide_kind),
                                    region_ptr, C.c_size_t(region_pitch), C.c_int(flags), C.c_int(rows), C.c_int(cols), C.c_int(0), C.byref(params), None)
    rp = C.c_void_p(r.data_ptr())
    assert solve(rp, r.stride(0), 4) == 1 and solve(rp, r.stride(0), -1) == 1 and solve(rp, r.stride(0), 7) == 1       # unknown flag bits
    assert solve(None, r.stride(0), rr.CUT) == 1                                       # null regions with flags
    assert solve(rp, cols - 1, rr.CUT) == 1 and solve(rp, cols - 1, 0) == 1            # a region pitch smaller than a row
    assert solve(rp, r.stride(0), rr.CUT, guide_kind=2) == 1                           # rtdd_solve_guided's: unknown guide kind ...
    assert solve(rp, r.stride(0), rr.CUT, guide_pitch=cols - 1) == 1                   # ... and a guide pitch smaller than a row
    out = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda:0")
    idx = lambda ptr, pitch, flags: L.rtdd_index_to_weight_regions(ctx._h, C.c_void_p(g.data_ptr()), C.c_size_t(g.stride(0)), C.c_int(GRAY), ptr, C.c_size_t(pitch),
                                                                   C.c_int(flags), C.c_void_p(d.data_ptr()), C.c_size_t(d.stride(0) * 4), C.c_void_p(out.data_ptr()),
                                                                   C.c_int(0), C.c_int(rows), C.c_int(cols))
    assert idx(rp, r.stride(0), 8) == 1 and idx(None, r.stride(0), rr.SMOOTH) == 1 and idx(rp, cols - 1, rr.SMOOTH) == 1
    codes_out = up(np.zeros((rows, cols), np.uint8)); e3 = up(np.zeros((rows, cols, 3), np.uint8))
    rc = lambda e, ep, mk, mp, level, o, op: L.rtdd_region_codes(ctx._h, e, C.c_size_t(ep), mk, C.c_size_t(mp), C.c_int(rows), C.c_int(cols), C.c_int(level), o, C.c_size_t(op))
    ev, mv, ov = C.c_void_p(e3.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(codes_out.data_ptr())
    assert rc(None, e3.stride(0), mv, m.stride(0), 0, ov, codes_out.stride(0)) == 1 and rc(ev, e3.stride(0), mv, m.stride(0), 0, None, codes_out.stride(0)) == 1
    assert rc(ev, cols * 3 - 1, mv, m.stride(0), 0, ov, codes_out.stride(0)) == 1 and rc(ev, e3.stride(0), mv, cols - 1, 0, ov, codes_out.stride(0)) == 1
    assert rc(ev, e3.stride(0), mv, m.stride(0), 0, ov, cols - 1) == 1 and rc(ev, e3.stride(0), mv, m.stride(0), -1, ov, codes_out.stride(0)) == 1
    ctx.synchronize()
    assert_bit_equal(down(d), depth, "a refused solve wrote the depth map")
    assert not out.any() and not down(codes_out).any()
    assert solve(rp, r.stride(0), rr.CUT) == 0                                         # the legal call still works
    ctx.synchronize()
    with rt.Context(0) as c:
        assert L.rtdd_pyramid_set_regions(c._h, C.c_int(rr.CUT)) == 2                  # no pyramid: RTDD_ERR_STATE
        assert L.rtdd_pyramid_regions(c._h) == 0 and L.rtdd_pyramid_regions_changed(c._h) == 2
        assert c.pyramid_create(ROWS, COLS) == 3
        ptr = C.c_void_p()
        img = lambda kind, level: L.rtdd_pyramid_image(c._h, C.c_int(kind), C.c_int(level), C.byref(ptr), None, None, None)
        for kind in (rt.IMG_REGION_EDITED, rt.IMG_REGION_MASK, rt.IMG_REGION_CODE):
            assert img(kind, 0) == 2                                                    # before the first set_regions: RTDD_ERR_STATE
        assert L.rtdd_pyramid_regions_changed(c._h) == 2
        assert L.rtdd_pyramid_set_regions(c._h, C.c_int(4)) == 1                        # unknown flag bits
        c.pyramid_set_regions(0)                                                        # (0 allocates nothing)
        assert img(rt.IMG_REGION_CODE, 0) == 2
        c.pyramid_set_regions(rr.SMOOTH)
        assert c.pyramid_regions() == rr.SMOOTH
        assert img(rt.IMG_REGION_EDITED, 0) == 0 and img(rt.IMG_REGION_MASK, 0) == 0 and img(rt.IMG_REGION_CODE, 2) == 0
        assert img(rt.IMG_REGION_EDITED, 1) == 1 and img(rt.IMG_REGION_MASK, 2) == 1    # level 0 only
        c.pyramid_set_regions(0)
        assert img(rt.IMG_REGION_CODE, 1) == 0 and c.pyramid_regions() == 0             # (the images are kept)
        c.pyramid_regions_changed()


# ---- 12. the harness -------------------------------------------------------------------------------------------------------------------------
def test_harness_region_flags(tmp_path, refs):
    write_pnm(tmp_path / "img.ppm", refs["bgr"][..., ::-1]); write_pnm(tmp_path / "ann.pgm", refs["ann"])
    fill = ";".join(f"{x},{y}" for x, y in POLYGON) + ":1"
    wand = f"{WAND[0]},{WAND[1]},{WAND[2]}:2"
    said, _, depth_map = run_harness(tmp_path, "pnm", ["--regions", "both", "--region-fill", fill, "--region-wand", wand, "--iters", str(ITERS), "--effect", "haze"])
    assert f"region 2, {int((refs['gray'].codes(0) == 2).sum())} pixels" in said, said
    assert np.array_equal(depth_map, refs["gray"].depth_u8)
    _, _, depth_map = run_harness(tmp_path, "pnm", ["--regions", "both", "--region-fill", fill, "--region-wand", wand, "--edges", "color", "--iters", str(ITERS), "--effect", "haze"])
    assert np.array_equal(depth_map, refs["colour"].depth_u8)
    _, _, depth_map = run_harness(tmp_path, "pnm", ["--iters", str(ITERS), "--effect", "haze"])
    assert np.array_equal(depth_map, refs["plain"].depth_u8)
    # region paints without --regions would be ignored: refused instead
    lone = subprocess.run([harness_bin()] + harness_files(tmp_path, "pnm") + ["--region-fill", fill], capture_output=True, text=True)
    assert lone.returncode == 1 and "need --regions" in lone.stdout, lone.stdout
