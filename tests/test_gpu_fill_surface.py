"""rtdd_fill_surface on the GPU, through the C ABI (-m gpu): every comparison is byte equality of both images, padding included, against
tests/surface_ref.py, plus the covered pixel count and the bounding box, and the pass count against the restated tiles' (an upper bound).
The shapes are rtdd_fill_similar's: one ragged word across and two blocks down with a ragged last block (67 x 45), four words by three
blocks (150 x 200), three words by one block (37 x 150), and a two-pixel-wide image 2000 rows long: a path through the V links alone, over
many rounds of passes."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import remove_ref as rmr
import roi_util
import strokes_ref as sr
import surface_ref as sf
import wand_ref as wr
from cascade_ref import Cascade
from gpu_util import bits, down, up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _assert_pyramid, _Dev, _pair, raw_target, sub_views

pytestmark = pytest.mark.gpu
f32 = np.float32


def _pair_of(rows, cols, seed):
    """An original, an edited image that is not the original (an erasure shows) and a scribble image with labels in it."""
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    ed = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    scr = np.zeros((rows, cols), np.uint8)
    scr[::3, ::4] = 255
    return orig, ed, scr


def _check(c, depth, wand, seed=0, what="", covered=sf.covered_queue, most_passes=None):
    rows, cols = depth.shape
    erases = wand[10] == sf.STROKE_ERASE
    orig, ed, scr = _pair_of(rows, cols, seed)
    o, e, s, d = _Dev(orig), _Dev(ed), _Dev(scr), _Dev(depth.view(np.uint8))
    info = c.fill_surface(wand, e.img, s.img, rows, cols, d.img, o.img if erases else None)      # (synchronises itself)
    want = sf.fill_surface(wand, ed, scr, depth, orig, covered)
    got_e, got_s = e.host(), s.host()
    got = (info.pixels, info.x0, info.y0, info.x1, info.y1)
    print(f"{what}{rows}x{cols}, wand {wand}: scribble differs at {int((got_s != scr).sum())}, edited at {int((got_e != ed).any(-1).sum())} pixels; info {got} "
          f"against {want}; {info.passes} passes" + (f" (at most {most_passes})" if most_passes is not None else ""))
    assert np.array_equal(got_s, scr) and np.array_equal(got_e, ed), what
    assert got == want, what
    assert np.array_equal(o.host(), orig) and np.array_equal(d.host(), depth.view(np.uint8)), "an input was written"
    if wand[5] & sf.SURFACE_GLOBAL:
        assert info.passes == 0
    else:
        assert 1 <= info.passes <= (most_passes if most_passes is not None else rows * cols + 1)
    return info


# ---- random fields, one word across and two blocks down: 67 x 45 -------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, sf.SURFACE_GLOBAL], ids=["connected", "global"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["constant", "ramp", "erase"])
def test_random_fields_one_word_wide(ctx, flags, kind):
    rows, cols = 67, 45
    assert sf.SEEDS_67x45 == [(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1), (20, 63), (21, 64), (44, 30)]
    sizes = []
    for i, depth, head in sf.random_cases(10 + kind, flags):             # default_rng(10), (11), (12): checked on the CPU to be not vacuous
        wand = sf.kinds(*head, rows, cols)[kind]
        sizes.append(_check(ctx, depth, wand, 20 + i).pixels)
    assert max(sizes) > rows * cols // 3 and len(set(sizes)) > 4


def test_random_fields_with_word_and_block_borders(ctx):
    """Seeds at (63, y) and (64, y), the two sides of a word's border, at both sides of a block's, and at the four corners of 150 x 200."""
    rows, cols = 150, 200
    rng = np.random.default_rng(30)
    for i, (x, y) in enumerate([(63, 10), (64, 10), (63, 64), (64, 63), (127, 128), (0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)]):
        depth = sf.field(rng, rows, cols)
        below, above = sf.BANDS[i % 6]
        _check(ctx, depth, sf.kinds(x, y, sf.STEPS[i % 6], below, above, 0, rows, cols)[i % 3], 40 + i, covered=sf.covered_graph)


# ---- paths that wind through the blocks ----------------------------------------------------------------------------------------------------
def test_a_spiral_needs_more_than_one_round_of_passes(ctx):
    rows, cols = 150, 200
    sp = wr.spiral(rows, cols)
    depth = sf.from_mask(sp)
    wand = (0, 0, 4.0, 255, 255, 0, 0, 0, cols - 1, rows - 1, 10, 240)
    m, passes = sf.covered_tiled(depth, wand)
    assert np.array_equal(m, sp) and passes > rt.WAND_ROUND           # (the restated tiles: the host loop's second round runs)
    info = _check(ctx, depth, wand, 50, "spiral: ", most_passes=passes)
    assert info.pixels == sp.sum()
    inner = tuple(int(v) for v in np.argwhere(sp & (np.abs(np.arange(rows)[:, None] - rows // 2) < 3))[-1][::-1])      # a seed deep inside: the path runs both ways
    _check(ctx, depth, sf.erase(*inner, 4.0), 51, "spiral from inside: ", covered=sf.covered_graph)


@pytest.mark.parametrize("rows,cols", [(150, 200), (37, 150)])
@pytest.mark.parametrize("direction", ["left", "right", "up", "down"])
def test_a_comb_is_entered_in_every_direction(ctx, rows, cols, direction):
    cm = wr.comb(rows, cols, direction)
    x, y = wr.comb_seed(rows, cols, direction)
    depth = sf.from_mask(cm)
    wand = sf.constant(x, y, 4.0, 33)
    m, passes = sf.covered_tiled(depth, wand)
    assert np.array_equal(m, cm)
    assert _check(ctx, depth, wand, 60, f"comb {direction}: ", covered=sf.covered_graph, most_passes=passes).pixels == cm.sum()


def test_a_long_vertical_path(ctx):
    """2000 x 2: a ramp of 0.1 per row down the left column, a wall down the right one; 32 blocks in a line, many rounds."""
    rows, cols = 2000, 2
    depth = np.empty((rows, cols), f32)
    depth[:, 0] = (np.arange(rows) * 0.1).astype(f32)
    depth[:, 1] = 250
    depth[-1, 1] = depth[-1, 0]                                       # ... and round the corner at the bottom
    wand = (0, 0, 0.125, 255, 255, 0, 0, 0, 0, rows - 1, 0, 255)
    m, passes = sf.covered_tiled(depth, wand)
    info = _check(ctx, depth, wand, 90, "long: ", covered=lambda d, w: m, most_passes=passes)
    assert info.pixels == rows + 1 and info.passes > rt.WAND_ROUND and (info.x1, info.y1) == (1, rows - 1)
    assert np.array_equal(sf.covered_graph(depth, wand), m)
    _check(ctx, depth, sf.erase(1, rows - 1, 0.125), 91, "long, from the far end: ", covered=lambda d, w: m)


# ---- what an eligibility plane cannot express ----------------------------------------------------------------------------------------------
def test_links_are_not_a_property_of_one_pixel(ctx):
    yy, xx = np.mgrid[:20, :30]
    board = np.where((yy + xx) & 1, f32(104), f32(100)).astype(f32)
    assert _check(ctx, board, sf.constant(7, 7, 3, 1), 100, "checkerboard, step 3: ").pixels == 1
    assert _check(ctx, board, sf.constant(7, 7, 4, 1), 101, "checkerboard, step 4: ").pixels == 600
    col = np.mgrid[:10, :70][1]
    assert _check(ctx, (f32(2) * col).astype(f32), sf.constant(35, 3, 2, 1, 10, 10), 102, "slope 2: ").pixels == 110
    assert _check(ctx, (f32(2.5) * col).astype(f32), sf.constant(35, 3, 2, 1, 10, 10), 103, "slope 2.5: ").pixels == 10
    stairs = (f32(50) + f32(5) * (np.mgrid[:12, :60][1] // 10)).astype(f32)
    info = _check(ctx, stairs, sf.constant(25, 5, 3, 1), 104, "terraces: ")
    assert (info.pixels, info.x0, info.x1) == (120, 20, 29)


def test_exact_thresholds(ctx):
    row = np.array([[100, 103, np.nextafter(f32(106), f32(np.inf)), 50]], f32)
    info = _check(ctx, row, sf.constant(0, 0, 3, 1), 110, "step: ")
    assert (info.pixels, info.x1) == (2, 1)
    lo, hi = f32(100) - f32(7), f32(100) + f32(9)
    edge = np.array([[np.nextafter(lo, f32(-np.inf)), lo, 100, hi, np.nextafter(hi, f32(np.inf))]], f32)
    for flags in (0, sf.SURFACE_GLOBAL):
        info = _check(ctx, edge, sf.constant(2, 0, 255, 1, 7, 9, flags), 111, "band: ")
        assert (info.pixels, info.x0, info.x1) == (3, 1, 3)


def test_special_values(ctx):
    rows, cols = 30, 70
    depth = sf.special_field(np.random.default_rng(7), rows, cols)
    wand = sf.constant(3, 5, 0, 1, 0, 0)                              # a NaN seed, step = below = above = 0
    m = sf.covered_queue(depth, wand)
    assert m[5, 3:8].all() and not m[6, 5] and (sf.clamped(depth)[m] == 0).all()
    assert _check(ctx, depth, wand, 120, "NaN seed: ").pixels == m.sum() >= 5
    g = _check(ctx, depth, wand[:5] + (sf.SURFACE_GLOBAL,) + wand[6:], 121, "NaN seed, global: ")
    assert g.pixels == (sf.clamped(depth) == 0).sum() > m.sum()
    for k, (x, y, step) in enumerate(((40, 20, 255), (10, 10, 2.5), (60, 3, 100))):
        _check(ctx, depth, sf.kinds(x, y, step, 255, 255, 0, rows, cols)[k], 122 + k, "special: ")


# ---- sub-image views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(roi_util.LAYOUTS_U8)), ids=lambda k: f"u8{roi_util.LAYOUTS_U8[k]}_f32{roi_util.LAYOUTS_F32[k]}")
def test_sub_image_views(ctx, k):
    """All four images inside larger allocations: odd lead bytes and pitches for the u8 images, a depth pointer aligned to 4 only; nothing
    outside the views is written, nothing uncovered inside them, the depth map and the original not at all; no original unless erasing."""
    rows, cols = 37, 75
    layout, (dlead, dres) = roi_util.LAYOUTS_U8[k], roi_util.LAYOUTS_F32[k]
    rng = np.random.default_rng(100 + k)
    for j, kind in enumerate((1, 2)):
        depth = sf.field(rng, rows, cols)
        orig, ed, scr = _pair_of(rows, cols, 100 + j)
        wand = sf.kinds(70, 20, 5.0, 6, 6, 0, rows, cols)[kind]                 # (checked on the CPU: 1930 .. 2745 of the 2775 pixels)
        o, e, s = sub_views(orig, ed, scr, layout)
        d = roi_util.Roi(depth, dlead, roi_util.pitch_for(cols * 4, dlead, dres), roi_util.FILL_INPUT, what="depth")
        info = ctx.fill_surface(wand, e.img, s.img, rows, cols, d.img, o.img if kind == 2 else None)
        want = sf.fill_surface(wand, ed, scr, depth, orig)
        assert np.array_equal(e.result(), ed) and np.array_equal(s.result(), scr), j
        o.assert_unchanged(); d.assert_unchanged()
        assert (info.pixels, info.x0, info.y0, info.x1, info.y1) == want and 1 < info.pixels < rows * cols


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    depth = sf.field(np.random.default_rng(4), rows, cols)
    orig, ed, scr = _pair_of(rows, cols, 4)
    o, e, s, d = _Dev(orig), _Dev(ed), _Dev(scr), _Dev(depth.view(np.uint8))
    L = rt.lib()
    names = [n for n, _ in rt.SurfaceWand._fields_]

    def W(**kw):
        f = dict(x=5, y=6, step=2.5, below=255.0, above=255.0, flags=0, ax0=0, ay0=0, ax1=30, ay1=15, label0=3, label1=200); f.update(kw)
        return rt.SurfaceWand(*(f[k] for k in names))

    def call(wand=W(), edited=e.img, scribble=s.img, original=o.img, dep=d.img, r=rows, c=cols, info=True):
        out = rt.WandInfo()
        t = raw_target(edited, scribble, original, r, c)
        dd = dep or (None, 0)
        return L.rtdd_fill_surface(ctx._h, C.byref(wand) if wand is not None else None, *t[:6], C.c_void_p(dd[0]), C.c_size_t(dd[1]), *t[6:],
                                   C.byref(out) if info else None)

    nan, inf = float("nan"), float("inf")
    refused = {
        "null wand": call(wand=None),
        "null depth": call(dep=None),
        "depth pitch below a row": call(dep=(d.img[0], cols * 4 - 4)),
        "depth pitch no multiple of 4": call(dep=(d.img[0], d.img[1] + 2)),
        "depth pointer at 2": call(dep=(d.img[0] + 2, d.img[1])),
        "depth pointer at 1": call(dep=(d.img[0] + 1, d.img[1])),
        "seed x < 0": call(W(x=-1)),
        "seed x == cols": call(W(x=cols)),
        "seed y < 0": call(W(y=-1)),
        "seed y == rows": call(W(y=rows)),
        "no rows": call(W(x=0, y=0), r=0),
        "no cols": call(W(x=0, y=0), c=0),
        "step NaN": call(W(step=nan)), "step inf": call(W(step=inf)), "step < 0": call(W(step=-0.5)), "step > 255": call(W(step=255.5)),
        "below NaN": call(W(below=nan)), "below inf": call(W(below=inf)), "below < 0": call(W(below=-1.0)), "below > 255": call(W(below=256.0)),
        "above NaN": call(W(above=nan)), "above -inf": call(W(above=-inf)), "above < 0": call(W(above=-1.0)), "above > 255": call(W(above=256.0)),
        "flag 2": call(W(flags=2)),
        "flag 3": call(W(flags=3)),
        "flag -1": call(W(flags=-1)),
        "ax0 too small": call(W(ax0=-32769)),
        "ay0 too large": call(W(ay0=32768)),
        "ax1 too large": call(W(ax1=32768)),
        "ay1 too small": call(W(ay1=-32769)),
        "label0 256": call(W(label0=256)),
        "label1 256": call(W(label1=256)),
        "label0 -2": call(W(label0=-2)),
        "label1 -2": call(W(label1=-2)),
        "only label0 erases": call(W(label0=-1)),
        "only label1 erases": call(W(label1=-1)),
        "erasing without original": call(W(label0=-1, label1=-1), original=None),
        "erasing with a short original pitch": call(W(label0=-1, label1=-1), original=(o.img[0], cols * 3 - 1)),
        "null edited": call(edited=None),
        "null scribble": call(scribble=None),
        "negative rows": call(r=-1),
        "negative cols": call(c=-1),
        "edited pitch": call(edited=(e.img[0], cols * 3 - 1)),
        "scribble pitch": call(scribble=(s.img[0], cols - 1)),
        "rows above 32768": call(r=32769),
        "cols above 32768": call(c=32769, edited=(e.img[0], 1 << 20), scribble=(s.img[0], 1 << 20), original=(o.img[0], 1 << 20), dep=(d.img[0], 1 << 20)),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr) and np.array_equal(d.host(), depth.view(np.uint8))
    assert ctx.get_option(rt.OPT_PENDING_CALLS) == 0                  # nothing was logged: a paint call, and a refused one
    assert call() == 0 and call(info=False) == 0 and call(original=None) == 0 and call(W(label0=-1, label1=-1)) == 0
    assert call(W(flags=1, step=0.0, below=0.0, above=0.0)) == 0 and call(W(step=255.0, below=255.0, above=255.0)) == 0
    assert call(W(ax0=-32768, ay0=32767, ax1=32767, ay1=-32768, label0=255, label1=0)) == 0
    assert ctx.get_option(rt.OPT_PENDING_CALLS) == 0
    with pytest.raises(rt.RtddError):
        ctx.fill_surface((5, 6, 1.0, 0, 0, 0, 0, 0, 1, 1, -1, 7), e.img, s.img, rows, cols, d.img, o.img)


# ---- on a pyramid --------------------------------------------------------------------------------------------------------------------------
_refs = {}


def _wands(ann, erasing):
    """A painting selection around the middle of the image; erasing: one that removes every label on pixels about as deep as a labelled
    one (global), that pixel included."""
    rows, cols = ann.shape
    out = [(cols // 2, rows // 2, 2.0, 20, 20, 0, cols // 2, 0, cols // 2, rows - 1, 200, 40)]
    if erasing:
        y, x = (int(v[0]) for v in np.nonzero(ann != 32))
        out.append(sf.erase(x, y, 0, 4, 4, sf.SURFACE_GLOBAL))
    return out


def _reference(oracle, lut, erasing):
    """The reduced pair: estimate, the wands on the estimate's own depth map, estimate."""
    if erasing not in _refs:
        bgr, ann = _pair()
        ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
        ref.estimate(ITERS)
        before = ref.scribble[0].copy()
        depth = ref.depth[0].copy()
        for wand in _wands(ann, erasing):
            sf.fill_surface(wand, ref.edited[0], ref.scribble[0], depth, bgr, sf.covered_graph)
        assert ((before != 255) & (ref.scribble[0] == 255)).sum() > 200
        if erasing:
            assert ((before == 255) & (ref.scribble[0] == 0)).sum() >= 1
            sr.rebuild(ref)                                           # the erasing call asks for the rebuild itself
        ref.estimate(ITERS)
        _refs[erasing] = ref
    return _refs[erasing]


@pytest.mark.parametrize("erasing", [False, True], ids=["painting", "erasing"])
def test_wands_on_the_annotation_pair_between_two_estimates(oracle, lut, erasing):
    """estimate queued, the wands on RTDD_IMG_DEPTH, estimate again, with no synchronisation of the test's own between them"""
    bgr, ann = _pair()
    rows, cols = ann.shape
    ref = _reference(oracle, lut, erasing)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == ref.P
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS)
        sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0)[:2]; ep = c.pyramid_image(rt.IMG_EDITED, 0)[:2]
        op = c.pyramid_image(rt.IMG_ORIGINAL, 0)[:2]; dp = c.pyramid_image(rt.IMG_DEPTH, 0)[:2]
        for wand in _wands(ann, erasing):
            assert c.fill_surface(wand, ep, sp, rows, cols, dp, op).pixels >= 1
        c.estimate_depth(ITERS); c.synchronize()
        _assert_pyramid(c, ref, "erasing" if erasing else "painting")
    if erasing:                                                       # not vacuous: without the rebuild the coarse levels keep the erased labels
        kept = _reference(oracle, lut, False)
        assert any((ref.scribble[l] != kept.scribble[l]).any() for l in range(1, ref.P))


def test_behind_an_unsynchronised_estimate_into_the_region_pair_then_removed():
    bgr, ann = _pair()
    rows, cols = ann.shape
    wand = (cols // 2, rows // 2, 2.0, 20, 20, 0, 0, 0, 0, 0, 5, 5)
    R = rmr.removal(0, 2, 0.0)
    got = []
    for synchronise in (False, True):
        with rt.Context(0) as c:
            c.GPULoadWeights(0.4)
            c.pyramid_create(rows, cols)
            c.pyramid_set_regions(rt.REGION_CUT)
            c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
            c.estimate_depth(ITERS)
            if synchronise:
                c.synchronize()
            e, m = c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2]
            o, d = c.pyramid_image(rt.IMG_ORIGINAL)[:2], c.pyramid_image(rt.IMG_DEPTH)[:2]
            info = c.fill_surface(wand, e, m, rows, cols, d)          # no original: it paints
            art, z = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), f32))
            c.remove_object(o, d, m, art, z, rows, cols, rt.Removal(**R))
            c.synchronize()
            got.append((c.pyramid_download(rt.IMG_DEPTH, 0), c.pyramid_download(rt.IMG_REGION_EDITED), c.pyramid_download(rt.IMG_REGION_MASK),
                        down(art), down(z), (info.pixels, info.x0, info.y0, info.x1, info.y1)))
    a, b = got
    assert all(np.array_equal(bits(x) if x.dtype == f32 else x, bits(y) if y.dtype == f32 else y) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]
    depth = a[0]
    ed, mask = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
    want = sf.fill_surface(wand, ed, mask, depth, None, sf.covered_graph)
    assert a[5] == want and 200 < want[0] < rows * cols // 2
    assert np.array_equal(a[1], ed) and np.array_equal(a[2], mask)
    art, z = rmr.remove(bgr, depth, mask, R)
    assert np.array_equal(a[3], art) and rmr.same_bits(a[4], z)
    assert not np.array_equal(art, bgr)


def test_a_retired_live_pointer_is_refused():
    bgr, ann = _pair()
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann)); c.synchronize()
        old_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0)[:2]; old_e = c.pyramid_image(rt.IMG_EDITED, 0)[:2]; dp = c.pyramid_image(rt.IMG_DEPTH, 0)[:2]
        wand = sf.constant(50, 11, 0, 64)
        c.fill_surface(wand, old_e, old_s, rows, cols, dp)            # fine: still the pyramid's
        scr = rt.host_image((rows, cols)); ed = rt.host_image((rows, cols, 3)); out = rt.host_image((rows, cols))
        scr.a[...] = c.pyramid_download(rt.IMG_SCRIBBLE, 0); ed.a[...] = c.pyramid_download(rt.IMG_EDITED, 0)
        assert scr.a[11, 50] == 255 and (ed.a[11, 50] == 64).all()
        c.live_submit(scr.a, ed.a, out.a, 50); c.live_wait()
        with pytest.raises(rt.RtddError) as err:
            c.fill_surface(wand, old_e, old_s, rows, cols, dp)
        assert err.value.status == 2
        new_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0)[:2]; new_e = c.pyramid_image(rt.IMG_EDITED, 0)[:2]
        assert new_s[0] != old_s[0]
        c.fill_surface(sf.constant(50, 11, 0, 128), new_e, new_s, rows, cols, dp)
        assert (c.pyramid_download(rt.IMG_EDITED, 0)[11, 50] == 128).all()
        for x in (scr, ed, out):
            x.free()


# ---- the scratch ---------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_is_shared_with_the_defocus_table():
    """A table-path defocus, a surface wand (its bit planes overwrite the table and its zero padding), the same defocus: equal outputs."""
    rows, cols = 120, 200
    rng = np.random.default_rng(9)
    orig = wr.quantised(rng, rows, cols)
    depth = rng.uniform(0, 255, (rows, cols)).astype(f32)
    with rt.Context(0) as c:
        o, d = up(orig), up(depth)
        c.set_option(rt.OPT_DEFOCUS_PATH, 1)
        outs = []
        for step in range(2):
            art = up(np.zeros_like(orig))
            c.GPUSimulateDefocus(o, d, art, rows, cols)
            c.synchronize()
            assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
            outs.append(down(art))
            if step == 0:
                _check(c, sf.field(rng, rows, cols), sf.constant(100, 60, 7.5, 200), 110, "between the two defocus calls: ", covered=sf.covered_graph)
        assert np.array_equal(outs[0], outs[1])
