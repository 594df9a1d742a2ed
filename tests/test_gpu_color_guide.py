"""The colour guide on the GPU (-m gpu): rtdd_index_to_weight_guided, rtdd_solve_guided, rtdd_pyrdown_bgr and the pyramid's guide
(rtdd_pyramid_set_guide) against the restatement of tests/color_guide_ref.py, bit for bit.

Shapes of the index pass and the solve: 1x1, 1x7, 9x1, 5x67, 33x130, 6x256, 6x257, 6x260, 7x515 -- ragged groups of four pixels and both
sides of the 256-pixel span of one workgroup's four-pixel threads.  Levels: (2 of 2) un-gated, (1 of 2) gated with threshold 4, (0 of 2)
gated with threshold 0; the depth maps have neighbouring u8 differences 0, 2, 3, 5, 6, 7 and 10, so both thresholds cut both ways
(asserted on the CPU for every shape that has an edge; 1x1 has none).  Estimates: 181 x 243 (three levels, odd sizes: the ceil chain of
the guide and the floor chain of the depth differ), maxIterations 64.  Every comparison of two GPU results is accompanied by a comparison
of one of them with the CPU restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_restatement as npr
import realtimedepthdiffusion_amd as rt
from cascade_ref import Cascade
from color_guide_ref import BGR, GRAY, ColorCascade, index_maps_bgr, isoluminant_image, solve_bgr
from effect_gpu import run_harness, write_pnm
from gpu_util import assert_bit_equal, down, up
from roi_util import Roi, pitch_for

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 7), (9, 1), (5, 67), (33, 130), (6, 256), (6, 257), (6, 260), (7, 515)]
SHAPE_IDS = [f"{r}x{c}" for r, c in SHAPES]
REGIMES = [(2, 2), (1, 2), (0, 2)]              # (level, maxLevel)
ROWS, COLS, ITERS = 181, 243, 64                # the estimates


@pytest.fixture(scope="module")
def ctx():
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        yield c


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _guide(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def _depth(rows, cols, seed):
    """u8 values 100 + cx[x % 7] + cy[y % 6] under a fraction in [0, 0.9): horizontal neighbours differ by 0, 3, 6, 0, 5, 6, 10 and
    vertical ones by 0, 2, 6, 0, 7, 1 after the truncating cast."""
    cx = np.array([0, 0, 3, 9, 9, 4, 10]); cy = np.array([0, 0, 2, 8, 8, 1])
    d = 100 + cx[np.arange(cols) % 7][None, :] + cy[np.arange(rows) % 6][:, None]
    return (d + np.random.default_rng(seed).uniform(0, 0.9, (rows, cols))).astype(np.float32)


def _assert_both_thresholds_cut_both_ways(depth):
    d = np.trunc(depth).astype(np.int32)
    diffs = np.concatenate([np.abs(d[:, 1:] - d[:, :-1]).ravel(), np.abs(d[1:] - d[:-1]).ravel()])
    if depth.size == 1:
        assert diffs.size == 0                      # one pixel: no edge for a threshold to cut
        return
    assert (diffs == 0).any() and ((diffs > 0) & (diffs <= 4)).any() and (diffs > 4).any(), sorted(set(diffs.tolist()))


def _mask(rows, cols, seed):
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((rows, cols)) < 0.12, 255, 32).astype(np.uint8)
    m[rows // 2, cols // 2] = 255
    return m


def _problem(rows, cols, seed):
    """(depth with random labels on its Dirichlet pixels, scribble mask, BGR guide)"""
    depth, mask = _depth(rows, cols, seed), _mask(rows, cols, seed + 1)
    lab = np.random.default_rng(seed + 2).integers(0, 256, (rows, cols)).astype(np.float32)
    depth[mask == 255] = lab[mask == 255]
    assert (mask == 255).any()
    return depth, mask, _guide(rows, cols, seed + 3)


def _allocate(c, rows, cols, level, max_level):
    c.GPUAllocateDeviceMemory(rows << level, cols << level, max_level + 1)


# ---- 1. the index pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_index_pass_matches_the_restatement(ctx, shape):
    rows, cols = shape
    bgr, depth = _guide(rows, cols, 10 + cols), _depth(rows, cols, 20 + cols)
    _assert_both_thresholds_cut_both_ways(depth)
    g, d = up(bgr), up(depth)
    for level, max_level in REGIMES:
        _allocate(ctx, rows, cols, level, max_level)
        out = torch.full((rows, cols, 2), -1, dtype=torch.int32, device="cuda:0")
        ctx.index_to_weight_guided(g, rt.GUIDE_BGR, d, out, level, rows, cols)
        ctx.synchronize()
        want = npr.pack_index(index_maps_bgr(bgr, depth, level, max_level))
        assert np.array_equal(out.cpu().numpy(), want), f"{rows}x{cols} level {level} of {max_level}"
    # the gray kind of the same entry point is rtdd_index_to_weight
    gray = np.ascontiguousarray(bgr[..., 1])
    a = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda:0")
    ctx.index_to_weight_guided(up(gray), rt.GUIDE_GRAY, d, a, 0, rows, cols)
    ctx.synchronize()
    assert np.array_equal(a.cpu().numpy(), npr.pack_index(npr.index_maps(gray, depth, 0, 2)))


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_guided_solve_matches_the_restatement(ctx, lut, shape):
    rows, cols = shape
    depth, mask, bgr = _problem(rows, cols, 40 + cols)
    m, g = up(mask), up(bgr)
    try:
        for level, max_level in REGIMES:
            _allocate(ctx, rows, cols, level, max_level)
            for contract in (1, 0):
                want = solve_bgr(depth, mask, bgr, 40, level, max_level, lut, contract)
                ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                for kernel in (1, 2):
                    ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel)
                    d = up(depth)
                    assert ctx.solve_guided(d, m, g, rt.GUIDE_BGR, rows, cols, level, maxIterations=40)[0] == 40
                    ctx.synchronize()
                    assert ctx.last_solve_info().kernel == kernel
                    assert_bit_equal(down(d), want, f"{rows}x{cols} level {level} of {max_level} kernel {kernel} contract {contract}")
    finally:
        ctx.set_option(rt.OPT_SWEEP_KERNEL, 0); ctx.set_option(rt.OPT_FP_CONTRACT, 1)


# ---- 3. both prepare kernels: an aligned guide and a region of interest -----------------------------------------------------------------
# (lead bytes, pitch residue) of the guide: aligned (the four-pixel kernel), pointers off by 1..3 bytes, odd pitches (the scalar one)
GUIDE_LAYOUTS = [(0, 0), (1, 0), (2, 4), (3, 1), (0, 3), (1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_aligned_guide_and_region_of_interest_give_the_same_bits(ctx, lut, shape):
    rows, cols = shape
    depth, mask, bgr = _problem(rows, cols, 70 + cols)
    m = up(mask)
    for level, max_level in ((0, 0), (1, 2)):               # un-gated, and gated: the row below is read for the depth gate too
        _allocate(ctx, rows, cols, level, max_level)
        want = solve_bgr(depth, mask, bgr, 8, level, max_level, lut, 1)
        results = []
        for lead, residue in GUIDE_LAYOUTS:
            roi = Roi(bgr, lead, pitch_for(cols * 3, lead, residue), what=f"guide (lead {lead}, residue {residue})")
            assert (roi.ptr % 4 == 0 and roi.pitch % 4 == 0) == ((lead, residue) == (0, 0))
            d = up(depth)
            ctx.solve_guided(d, m, roi.img, rt.GUIDE_BGR, rows, cols, level, maxIterations=8)
            ctx.synchronize()
            roi.assert_unchanged()                          # (0xFF all around the view: a byte read from there would change an index)
            results.append(down(d))
        for (lead, residue), got in zip(GUIDE_LAYOUTS, results):
            assert_bit_equal(got, results[0], f"{rows}x{cols} level {level}: lead {lead}, residue {residue} against the aligned guide")
        assert_bit_equal(results[0], want, f"{rows}x{cols} level {level}: the aligned guide against the restatement")


def test_a_guide_row_may_end_its_allocation(ctx, lut):
    """A guide whose pitch is 3 * cols rounded up to 4 and whose last row ends where its allocation ends -- the tightest layout the
    four-pixel kernel is dispatched on, ragged last groups included: the bits are the restatement's."""
    for rows, cols in ((6, 260), (6, 257), (3, 4), (2, 5)):
        depth, mask, bgr = _problem(rows, cols, 90 + cols)
        _allocate(ctx, rows, cols, 0, 0)
        pitch = (cols * 3 + 3) // 4 * 4
        flat = torch.zeros(pitch * (rows - 1) + cols * 3, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(pitch * rows, np.uint8)
        host.reshape(rows, pitch)[:, :cols * 3] = bgr.reshape(rows, -1)
        flat.copy_(torch.from_numpy(host[:flat.numel()]))
        d = up(depth)
        ctx.solve_guided(d, up(mask), (flat.data_ptr(), pitch), rt.GUIDE_BGR, rows, cols, 0, maxIterations=8)
        ctx.synchronize()
        assert_bit_equal(down(d), solve_bgr(depth, mask, bgr, 8, 0, 0, lut, 1), f"{rows}x{cols}")


# ---- 4. identity through the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["jacobi", "rbgs", "multigrid"])
def test_gray_kind_is_solve_ex_and_replicated_gray_is_the_oracle(ctx, oracle, lut, method):
    rows, cols = 33, 130
    depth, mask, _ = _problem(rows, cols, 120)
    rng = np.random.default_rng(121)
    gray = (rng.integers(0, 256, (rows, cols)) // 4 + 90).astype(np.uint8)
    gray[rng.random((rows, cols)) < 0.2] = 7                     # some strong edges, denormal weights included
    bgr = np.repeat(gray[..., None], 3, axis=2)
    _allocate(ctx, rows, cols, 0, 0)
    kw = {"jacobi": dict(method=rt.METHOD_CHEBYSHEV_JACOBI, maxIterations=40), "rbgs": dict(method=rt.METHOD_RED_BLACK_GS, maxIterations=9),
          "multigrid": dict(method=rt.METHOD_MULTIGRID, maxIterations=2)}[method]
    want = depth.copy()
    if method == "jacobi":
        oracle.solve(want, mask, gray, 40, 0, 0, lut, 1)
    else:
        idx = oracle.index_to_weight(gray, depth, 0, 0)
        if method == "rbgs":
            for _ in range(9):
                oracle.rbgs_sweep(want, idx, mask, lut, 1)
        else:
            oracle.mg_solve(want, idx, mask, lut, 1, 2, 0.0, 1)
    m, g1, g3 = up(mask), up(gray), up(bgr)
    a, b, c3 = up(depth), up(depth), up(depth)
    ctx.solve_ex(a, m, g1, rows, cols, 0, **kw); info_a = ctx.last_solve_info()
    ctx.solve_guided(b, m, g1, rt.GUIDE_GRAY, rows, cols, 0, **kw); info_b = ctx.last_solve_info()
    ctx.solve_guided(c3, m, g3, rt.GUIDE_BGR, rows, cols, 0, **kw)
    ctx.synchronize()
    assert info_a.describe() == info_b.describe()
    assert_bit_equal(down(a), want, f"{method}: rtdd_solve_ex against the oracle")
    assert_bit_equal(down(b), down(a), f"{method}: the gray kind against rtdd_solve_ex")
    assert_bit_equal(down(c3), want, f"{method}: replicated gray as a BGR guide against the oracle")


# ---- 5. rtdd_pyrdown_bgr -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (45, 61), (181, 243)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyrdown_bgr_is_pyrdown_per_channel(ctx, oracle, shape):
    rows, cols = shape
    bgr = _guide(rows, cols, 130 + cols)
    dst = up(np.zeros(((rows + 1) // 2, (cols + 1) // 2, 3), np.uint8))
    ctx.pyrdown_bgr(up(bgr), rows, cols, dst)
    ctx.synchronize()
    got = down(dst)
    for ch in range(3):
        assert np.array_equal(got[..., ch], oracle.pyrdown_u8(bgr[..., ch].copy())), f"channel {ch}"
    # a source view with a foreign byte on every side
    roi = Roi(bgr, 1, pitch_for(cols * 3, 1, 3))
    dst2 = up(np.zeros_like(got))
    ctx.pyrdown_bgr(roi.img, rows, cols, dst2)
    ctx.synchronize()
    assert np.array_equal(down(dst2), got)
    roi.assert_unchanged()


# ---- 6. the estimate -----------------------------------------------------------------------------------------------------------------------
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


def _pair_annotation(rows=ROWS, cols=COLS):
    """One label on each side of the isoluminant pair's boundary."""
    ann = np.full((rows, cols), 32, np.uint8)
    ann[rows // 3: rows // 3 + 8, 12: 30] = 0
    ann[rows // 2: rows // 2 + 8, cols - 30: cols - 12] = 254
    return ann


@pytest.fixture(scope="module")
def refs(oracle, lut):
    """The CPU references the estimate tests share, computed once and left as they are."""
    t = min(8, oracle.max_threads())
    out = {"bgr": _blocks(1), "ann": _annotation(), "pair": isoluminant_image(ROWS, COLS), "pair_ann": _pair_annotation()}
    out["colour"] = ColorCascade(oracle, out["bgr"], out["ann"], lut, 1, t, guide=BGR); out["colour"].estimate(ITERS)
    out["pair_colour"] = ColorCascade(oracle, out["pair"], out["pair_ann"], lut, 1, t, guide=BGR); out["pair_colour"].estimate(ITERS)
    out["pair_constant"] = Cascade(oracle, np.full_like(out["pair"], 59), out["pair_ann"], lut, 1, t); out["pair_constant"].estimate(ITERS)
    return out


def _estimate(c, bgr, ann, guide, iters=ITERS, guide_first=True):
    levels = c.pyramid_create(bgr.shape[0], bgr.shape[1])
    if guide_first:
        c.pyramid_set_guide(guide)
    c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
    if not guide_first:
        c.pyramid_set_guide(guide)
    assert c.pyramid_guide() == guide
    c.estimate_depth(iters); c.synchronize()
    return levels


def _assert_levels(c, ref, what):
    for l in range(ref.P - 1, -1, -1):
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), ref.depth[l], f"{what}: depth level {l}")
    assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), ref.depth_u8), f"{what}: u8 map"


def test_estimate_under_the_colour_guide(ctx, refs):
    ref = refs["colour"]
    assert _estimate(ctx, refs["bgr"], refs["ann"], rt.GUIDE_BGR) == ref.P == 3
    _assert_levels(ctx, ref, "colour estimate")
    for l in range(ref.P):
        got = ctx.pyramid_download(rt.IMG_GUIDE_BGR, l)
        assert got.shape == ref.color[l].shape and np.array_equal(got, ref.color[l]), f"guide level {l}"
        assert np.array_equal(ctx.pyramid_download(rt.IMG_GRAY, l), ref.gray[l]), f"gray level {l}"
    assert ctx.pyramid_image(rt.IMG_GUIDE_BGR, 0)[0] == ctx.pyramid_image(rt.IMG_ORIGINAL, 0)[0]
    # and the guide matters on this image
    gray_ref_u8 = None
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _estimate(c, refs["bgr"], refs["ann"], rt.GUIDE_GRAY)
        gray_ref_u8 = c.pyramid_download(rt.IMG_DEPTH_U8)
    assert not np.array_equal(gray_ref_u8, ref.depth_u8)


def test_replicated_gray_estimates_alike_under_both_guides(ctx, oracle, lut, refs):
    gray = oracle.bgr2gray(refs["bgr"])
    bgr = np.repeat(gray[..., None], 3, axis=2)
    ref = Cascade(oracle, bgr, refs["ann"], lut, 1, threads=min(8, oracle.max_threads()))
    ref.estimate(ITERS)
    assert np.array_equal(ref.gray[0], gray)
    for guide in (rt.GUIDE_GRAY, rt.GUIDE_BGR):
        _estimate(ctx, bgr, refs["ann"], guide)
        _assert_levels(ctx, ref, f"replicated gray under guide {guide}")


def test_isoluminant_pair_gray_sees_a_constant_image_colour_does_not(ctx, refs):
    _estimate(ctx, refs["pair"], refs["pair_ann"], rt.GUIDE_GRAY)
    assert (ctx.pyramid_download(rt.IMG_GRAY, 0) == 59).all()
    _assert_levels(ctx, refs["pair_constant"], "the pair under the gray guide against a constant image")
    _estimate(ctx, refs["pair"], refs["pair_ann"], rt.GUIDE_BGR)
    _assert_levels(ctx, refs["pair_colour"], "the pair under the colour guide")
    assert not np.array_equal(refs["pair_colour"].depth_u8, refs["pair_constant"].depth_u8)


# ---- 7. state ------------------------------------------------------------------------------------------------------------------------------
def test_guide_state_follows_the_calls(oracle, lut):
    """91 x 123 (two levels), maxIterations 32: set_guide before and after set_image, toggled between estimates (which continue from each
    other's depth pyramid), and a second image under BGR."""
    rows, cols, iters = 91, 123, 32
    first, second = _blocks(7, rows, cols), _blocks(8, rows, cols)
    ann = _annotation(rows, cols)
    ref = ColorCascade(oracle, first, ann, lut, 1, 1, guide=BGR)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == ref.P == 2
        assert c.pyramid_guide() == rt.GUIDE_GRAY
        c.pyramid_set_guide(rt.GUIDE_BGR)                           # before any image
        c.pyramid_set_image(up(first)); c.pyramid_set_annotation(up(ann))
        for step, guide in enumerate((BGR, GRAY, BGR, BGR, GRAY)):
            c.pyramid_set_guide(guide)
            assert c.pyramid_guide() == guide
            c.estimate_depth(iters); c.synchronize()
            ref.guide = guide; ref.estimate(iters)
            _assert_levels(c, ref, f"estimate {step} under guide {guide}")
        # a new image while the guide is GRAY, then BGR again: the chain is built from the image as it is now
        c.pyramid_set_image(up(second)); c.pyramid_set_annotation(up(ann))
        c.pyramid_set_guide(rt.GUIDE_BGR)
        ref2 = ColorCascade(oracle, second, ann, lut, 1, 1, guide=BGR)
        c.estimate_depth(iters); c.synchronize(); ref2.estimate(iters)
        _assert_levels(c, ref2, "second image, guide set after it")
        assert np.array_equal(c.pyramid_download(rt.IMG_GUIDE_BGR, 1), ref2.color[1])
        # a new image while the guide is BGR: set_image rebuilds the chain
        c.pyramid_set_image(up(first)); c.pyramid_set_annotation(up(ann))
        ref3 = ColorCascade(oracle, first, ann, lut, 1, 1, guide=BGR)
        c.estimate_depth(iters); c.synchronize(); ref3.estimate(iters)
        assert np.array_equal(c.pyramid_download(rt.IMG_GUIDE_BGR, 1), ref3.color[1])
        _assert_levels(c, ref3, "first image again, set under BGR")
        # rtdd_refine_depth follows the guide: 5 more sweeps of level 0 (level 0 of 2: gated, threshold 0)
        c.refine_depth(method=rt.METHOD_CHEBYSHEV_JACOBI, maxIterations=5, tolerance=0.0)
        c.synchronize()
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, 0), solve_bgr(ref3.depth[0], ref3.scribble[0], first, 5, 0, 1, lut, 1), "refine under BGR")
        # a new pyramid starts with the gray guide again
        c.pyramid_create(rows, cols)
        assert c.pyramid_guide() == rt.GUIDE_GRAY


# ---- 8. a batch ------------------------------------------------------------------------------------------------------------------------------
def _info_tuple(c, level):
    info, n = c.pyramid_level_info(level)
    return (info.kernel, info.tile, info.temporal_depth, info.persistent, info.fp_contract, info.launches, info.iterations, n)


def test_batch_under_the_colour_guide(ctx, refs):
    images = [refs["bgr"], _blocks(2), _blocks(3)]
    anns = [refs["ann"], _annotation(shift=9), _annotation(shift=17)]
    singles = []
    for bgr, ann in zip(images, anns):
        levels = _estimate(ctx, bgr, ann, rt.GUIDE_BGR)
        singles.append(([ctx.pyramid_download(rt.IMG_DEPTH, l) for l in range(levels)], ctx.pyramid_download(rt.IMG_DEPTH_U8),
                        [ctx.pyramid_download(rt.IMG_GUIDE_BGR, l) for l in range(levels)]))
    assert_bit_equal(singles[0][0][0], refs["colour"].depth[0], "the first single-image estimate against the restatement")
    infos = {}
    for guide, guide_first in ((rt.GUIDE_GRAY, True), (rt.GUIDE_BGR, True), (rt.GUIDE_BGR, False)):
        with rt.Context(0) as c:
            c.GPULoadWeights(0.4)
            levels = c.pyramid_create_batch(ROWS, COLS, 3)
            if guide_first:
                c.pyramid_set_guide(guide)
            for b, (bgr, ann) in enumerate(zip(images, anns)):
                c.pyramid_select(b); c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
            if not guide_first:
                c.pyramid_set_guide(guide)                          # builds the chain of every image of the batch
            c.estimate_depth_batch(ITERS); c.synchronize()
            infos[(guide, guide_first)] = [_info_tuple(c, l) for l in range(levels)]
            if guide == rt.GUIDE_GRAY:
                continue
            for b in range(3):
                c.pyramid_select(b)
                for l in range(levels):
                    assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), singles[b][0][l], f"image {b} level {l}")
                    assert np.array_equal(c.pyramid_download(rt.IMG_GUIDE_BGR, l), singles[b][2][l]), f"image {b} guide level {l}"
                assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), singles[b][1]), f"image {b} u8 map"
    assert infos[(rt.GUIDE_BGR, True)] == infos[(rt.GUIDE_GRAY, True)] == infos[(rt.GUIDE_BGR, False)]


# ---- 9. live frames ------------------------------------------------------------------------------------------------------------------------
def test_live_frames_under_the_colour_guide(oracle, lut, refs):
    ref = refs["colour"]
    with rt.Context(0) as c:                                            # what rtdd_estimate_depth gives, frame by frame (warm starts)
        c.GPULoadWeights(0.4)
        _estimate(c, refs["bgr"], refs["ann"], rt.GUIDE_BGR)
        want = [c.pyramid_download(rt.IMG_DEPTH_U8)]
        c.estimate_depth(ITERS); c.synchronize()
        want.append(c.pyramid_download(rt.IMG_DEPTH_U8))
    assert np.array_equal(want[0], ref.depth_u8)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(ROWS, COLS)
        c.pyramid_set_guide(rt.GUIDE_BGR)
        c.pyramid_set_image(up(refs["bgr"])); c.synchronize()
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


# ---- 10. a healed time-out replays a guided call as guided -------------------------------------------------------------------------------
def test_healed_solve_and_estimate_keep_their_guide(lut, refs, capfd):
    rows, cols = 33, 130
    depth, mask, bgr = _problem(rows, cols, 150)
    want = solve_bgr(depth, mask, bgr, 24, 0, 0, lut, 1)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.GPUAllocateDeviceMemory(rows, cols, 1)
        d, m, g = up(depth), up(mask), up(bgr)
        c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
        c.solve_guided(d, m, g, rt.GUIDE_BGR, rows, cols, 0, maxIterations=24)
        assert c.last_solve_info().kernel == 2
        c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        assert_bit_equal(down(d), want, "healed guided solve")
    ref = refs["colour"]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(ROWS, COLS)
        c.pyramid_set_guide(rt.GUIDE_BGR)
        c.pyramid_set_image(up(refs["bgr"])); c.pyramid_set_annotation(up(refs["ann"]))
        c.synchronize()
        c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
        c.estimate_depth(ITERS)
        c.pyramid_set_guide(rt.GUIDE_GRAY)                          # the replay must not look here
        c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        assert c.pyramid_guide() == rt.GUIDE_GRAY
        _assert_levels(c, ref, "healed colour estimate, the pyramid switched to gray before the synchronisation")
    capfd.readouterr()                                                  # (the heal's one warning on stderr)


# ---- 11. refusals, before any launch -------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rows, cols = 9, 21
    depth, mask, bgr = _problem(rows, cols, 170)
    _allocate(ctx, rows, cols, 0, 0)
    d, m, g = up(depth), up(mask), up(bgr)
    L = rt.lib()
    params = rt.SolveParams(rt.METHOD_CHEBYSHEV_JACOBI, 5, 0.0, 0, 0.0)

    def solve(guide_ptr, guide_pitch, kind):
        return L.rtdd_solve_guided(ctx._h, C.c_void_p(d.data_ptr()), C.c_size_t(d.stride(0) * 4), C.c_void_p(m.data_ptr()), C.c_size_t(m.stride(0)),
                                   guide_ptr, C.c_size_t(guide_pitch), C.c_int(kind), C.c_int(rows), C.c_int(cols), C.c_int(0), C.byref(params), None)
    gp = C.c_void_p(g.data_ptr())
    assert solve(gp, g.stride(0), 2) == 1 and solve(gp, g.stride(0), -1) == 1          # unknown kind
    assert solve(gp, cols * 3 - 1, rt.GUIDE_BGR) == 1                                  # BGR pitch below 3 * cols
    assert solve(gp, cols, rt.GUIDE_BGR) == 1                                          # (a gray image's pitch)
    assert solve(None, g.stride(0), rt.GUIDE_BGR) == 1                                 # null guide
    out = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda:0")
    idx = lambda ptr, pitch, kind: L.rtdd_index_to_weight_guided(ctx._h, ptr, C.c_size_t(pitch), C.c_int(kind), C.c_void_p(d.data_ptr()),
                                                                 C.c_size_t(d.stride(0) * 4), C.c_void_p(out.data_ptr()), C.c_int(0), C.c_int(rows), C.c_int(cols))
    assert idx(gp, g.stride(0), 5) == 1 and idx(gp, cols * 3 - 1, rt.GUIDE_BGR) == 1 and idx(None, g.stride(0), rt.GUIDE_BGR) == 1
    small = up(np.zeros(((rows + 1) // 2, (cols + 1) // 2, 3), np.uint8))
    assert L.rtdd_pyrdown_bgr(ctx._h, gp, C.c_size_t(cols * 3 - 1), C.c_int(rows), C.c_int(cols), C.c_void_p(small.data_ptr()), C.c_size_t(small.stride(0))) == 1
    assert L.rtdd_pyrdown_bgr(ctx._h, None, C.c_size_t(g.stride(0)), C.c_int(rows), C.c_int(cols), C.c_void_p(small.data_ptr()), C.c_size_t(small.stride(0))) == 1
    ctx.synchronize()
    assert_bit_equal(down(d), depth, "a refused solve wrote the depth map")
    assert not out.any()
    assert solve(gp, g.stride(0), rt.GUIDE_BGR) == 0                                   # the legal call still works
    ctx.synchronize()
    with rt.Context(0) as c:
        assert L.rtdd_pyramid_set_guide(c._h, C.c_int(rt.GUIDE_BGR)) == 2              # no pyramid: RTDD_ERR_STATE
        assert L.rtdd_pyramid_guide(c._h) == rt.GUIDE_GRAY
        assert c.pyramid_create(ROWS, COLS) == 3
        ptr = C.c_void_p()
        img = lambda level: L.rtdd_pyramid_image(c._h, C.c_int(rt.IMG_GUIDE_BGR), C.c_int(level), C.byref(ptr), None, None, None)
        assert img(0) == 0 and img(1) == 2 and img(2) == 2                              # no chain yet: RTDD_ERR_STATE above level 0
        assert L.rtdd_pyramid_set_guide(c._h, C.c_int(2)) == 1                          # unknown kind
        c.pyramid_set_guide(rt.GUIDE_BGR)
        assert img(1) == 0 and img(2) == 0
        c.pyramid_set_guide(rt.GUIDE_GRAY)
        assert img(2) == 0                                                              # (the allocation is kept)


# ---- 12. the harness -------------------------------------------------------------------------------------------------------------------------
def test_harness_edges_color(tmp_path, refs):
    write_pnm(tmp_path / "img.ppm", refs["pair"][..., ::-1]); write_pnm(tmp_path / "ann.pgm", refs["pair_ann"])
    _, _, depth_map = run_harness(tmp_path, "pnm", ["--edges", "color", "--iters", str(ITERS), "--effect", "haze"])
    assert np.array_equal(depth_map, refs["pair_colour"].depth_u8)
    _, _, depth_map = run_harness(tmp_path, "pnm", ["--edges", "gray", "--iters", str(ITERS), "--effect", "haze"])
    assert np.array_equal(depth_map, refs["pair_constant"].depth_u8)
