"""rtdd_fill_similar on the GPU, through the C ABI (-m gpu): every comparison is byte equality of both images, padding included, against
tests/wand_ref.py, plus the covered pixel count and the bounding box (or, for whole estimates, of every level against the restated cascade
fed with the restated annotation).  The shapes are the smallest at which the kernels can go wrong: one word across with a ragged last
word and two blocks down with a ragged last block (67 x 45), four words by three blocks and three words by one block (150 x 200,
37 x 150) for everything that crosses a block's border, and two-pixel-wide images as long as the domain for the index width and for
hundreds of passes."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import roi_util
import strokes_ref as sr
import wand_ref as wr
from cascade_ref import Cascade
from gpu_util import up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _assert_pyramid, _Dev, _pair, raw_target, sub_views

pytestmark = pytest.mark.gpu


def _pair_of(orig, seed):
    """An edited image that is not the original (an erasure shows) and a scribble image with labels in it (an erasure shows there too)."""
    rows, cols = orig.shape[:2]
    ed = np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    scr = np.zeros((rows, cols), np.uint8)
    scr[::3, ::4] = 255
    return ed, scr


def _check(c, orig, wand, seed=0, what="", covered=wr.covered_queue, most_passes=None):
    rows, cols = orig.shape[:2]
    ed, scr = _pair_of(orig, seed)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    info = c.fill_similar(wand, e.img, s.img, rows, cols, o.img)      # (synchronises itself)
    want = wr.fill_similar(wand, ed, scr, orig, covered)
    got_e, got_s = e.host(), s.host()
    got = (info.pixels, info.x0, info.y0, info.x1, info.y1)
    print(f"{what}{rows}x{cols}, wand {wand}: scribble differs at {int((got_s != scr).sum())}, edited at {int((got_e != ed).any(-1).sum())} pixels; info {got} "
          f"against {want}; {info.passes} passes" + (f" (at most {most_passes})" if most_passes is not None else ""))
    assert np.array_equal(got_s, scr) and np.array_equal(got_e, ed), what
    assert got == want, what
    assert np.array_equal(o.host(), orig)
    if wand[3] & wr.WAND_GLOBAL:
        assert info.passes == 0
    else:
        assert 1 <= info.passes <= (most_passes if most_passes is not None else rows * cols + 1)
    return info


def _kinds(x, y, tol, flags, rows, cols):
    """a constant label, a ramp across the image, an eraser"""
    return (wr.constant(x, y, tol, 77, flags), (x, y, tol, flags, 3, -4, cols - 5, rows + 6, 5, 250), wr.erase(x, y, tol, flags))


# ---- one word across, two blocks down: 67 x 45 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, wr.WAND_CONNECT_8, wr.WAND_GLOBAL, wr.WAND_GLOBAL | wr.WAND_CONNECT_8], ids=["4", "8", "global", "global8"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["constant", "ramp", "erase"])
def test_random_images_one_word_wide(ctx, flags, kind):
    rows, cols = 67, 45
    rng = np.random.default_rng(10 + 4 * kind + flags)
    seeds = [(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1), (20, 63), (21, 64), (44, 30)]      # the corners, both sides of the block border, the ragged word's last bit
    sizes = []
    for i, seed in enumerate(seeds + [None] * 5):
        orig = wr.quantised(rng, rows, cols)
        wand = wr.random_wand(rng, rows, cols, kind, flags, seed, wr.TOLERANCES[i % 6])
        sizes.append(_check(ctx, orig, wand, 20 + i).pixels)
    # not vacuous: tolerance 15 makes two of the three levels eligible at the least, which percolates (site threshold 0.593 under 4, 0.407
    # under 8); tolerances up to 3 keep one level, a third of the pixels: small components
    assert max(sizes) > rows * cols // 3 and len(set(sizes)) > 4


def test_random_images_with_block_borders_at_63_and_64(ctx):
    """Seeds at (63, y) and (64, y), the two sides of a word's border, and at the four corners of 150 x 200: four words by three blocks."""
    rows, cols = 150, 200
    rng = np.random.default_rng(30)
    for i, seed in enumerate([(63, 10), (64, 10), (63, 64), (64, 63), (127, 128), (0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)]):
        orig = wr.quantised(rng, rows, cols)
        x, y = seed
        tol = (3, 12, 15)[i % 3]
        _check(ctx, orig, _kinds(x, y, tol, (i % 2) * wr.WAND_CONNECT_8, rows, cols)[i % 3], 40 + i, covered=wr.covered_label)


# ---- paths that wind through the blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, wr.WAND_CONNECT_8], ids=["4", "8"])
def test_a_spiral_needs_more_than_one_round_of_passes(ctx, flags):
    rows, cols = 150, 200
    sp = wr.spiral(rows, cols)
    orig = wr.from_mask(sp)
    wand = (0, 0, 5, flags, 0, 0, cols - 1, rows - 1, 10, 240)
    m, passes = wr.covered_tiled(orig, wand)
    assert np.array_equal(m, sp) and passes > rt.WAND_ROUND          # (the restated tiles: the host loop's second round runs)
    info = _check(ctx, orig, wand, 50, "spiral: ", most_passes=passes)
    assert info.pixels == sp.sum()
    inner = tuple(int(v) for v in np.argwhere(sp & (np.abs(np.arange(rows)[:, None] - rows // 2) < 3))[-1][::-1])      # a seed deep inside: the path runs both ways
    _check(ctx, orig, wr.erase(*inner, 5, flags), 51, "spiral from inside: ")


@pytest.mark.parametrize("rows,cols", [(150, 200), (37, 150)])
@pytest.mark.parametrize("direction", ["left", "right", "up", "down"])
def test_a_comb_is_entered_in_every_direction(ctx, rows, cols, direction):
    cm = wr.comb(rows, cols, direction)
    x, y = wr.comb_seed(rows, cols, direction)
    orig = wr.from_mask(cm)
    for flags in (0, wr.WAND_CONNECT_8):
        wand = wr.constant(x, y, 5, 33, flags)
        m, passes = wr.covered_tiled(orig, wand)
        assert np.array_equal(m, cm)
        assert _check(ctx, orig, wand, 60, f"comb {direction}: ", most_passes=passes).pixels == cm.sum()


def _link(rows, cols, anti):
    """Two squares that touch only diagonally, across the block corner (63, 63) | (64, 64) (anti: (64, 63) | (63, 64))."""
    m = np.zeros((rows, cols), bool)
    if anti:
        m[50:64, 64:78] = True; m[64:80, 48:64] = True
        return m, (70, 55), (55, 70)
    m[50:64, 50:64] = True; m[64:80, 64:80] = True
    return m, (55, 55), (70, 70)


@pytest.mark.parametrize("anti", [False, True], ids=["main", "anti"])
def test_a_diagonal_link_across_a_block_corner(ctx, anti):
    rows, cols = 150, 200
    m, upper, lower = _link(rows, cols, anti)
    orig = wr.from_mask(m)
    for seed, own in ((upper, m & (np.arange(rows)[:, None] < 64)), (lower, m & (np.arange(rows)[:, None] >= 64))):
        assert _check(ctx, orig, wr.constant(*seed, 5, 9), 70, "apart under 4: ", covered=wr.covered_label).pixels == own.sum()
        assert _check(ctx, orig, wr.constant(*seed, 5, 9, wr.WAND_CONNECT_8), 71, "joined under 8: ", covered=wr.covered_label).pixels == m.sum()


@pytest.mark.parametrize("rows,cols", [(150, 200), (37, 150)])
def test_one_ineligible_column_or_row_at_64_separates(ctx, rows, cols):
    for flags in (0, wr.WAND_CONNECT_8):
        m = np.ones((rows, cols), bool); m[:, 64] = False
        assert _check(ctx, wr.from_mask(m), wr.constant(10, 10, 5, 9, flags), 80, "column 64, from the left: ", covered=wr.covered_label).pixels == 64 * rows
        assert _check(ctx, wr.from_mask(m), wr.erase(100, 10, 5, flags), 81, "column 64, from the right: ", covered=wr.covered_label).pixels == (cols - 65) * rows
        if rows > 65:
            m = np.ones((rows, cols), bool); m[64, :] = False
            assert _check(ctx, wr.from_mask(m), wr.constant(10, 10, 5, 9, flags), 82, "row 64, from above: ", covered=wr.covered_label).pixels == 64 * cols
            assert _check(ctx, wr.from_mask(m), wr.erase(10, 100, 5, flags), 83, "row 64, from below: ", covered=wr.covered_label).pixels == (rows - 65) * cols


# ---- the index width, hundreds of passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(2, 32768), (32768, 2)])
def test_images_as_long_as_the_domain(ctx, rows, cols):
    flat = np.full((rows, cols, 3), 90, np.uint8)
    whole = lambda o, w: np.ones((rows, cols), bool)
    info = _check(ctx, flat, (cols - 1, rows - 1, 0, 0, 0, 0, cols - 1, rows - 1, 0, 255), 90, "flat: ", covered=whole, most_passes=513)
    assert info.pixels == rows * cols and info.passes > rt.WAND_ROUND   # 512 blocks in a line, one pass each unless a racing read helps: many rounds
    _check(ctx, flat, wr.erase(0, 0, 0), 91, "flat, erased: ", covered=whole)
    board = np.where(((np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1).astype(bool)[..., None], np.uint8(90), np.uint8(91)).repeat(3, -1)
    assert _check(ctx, board, wr.constant(cols // 2, 1, 0, 200), 92, "checkerboard under 4: ", covered=wr.covered_label).pixels == 1
    half = _check(ctx, board, wr.constant(cols // 2, 1, 0, 200, wr.WAND_CONNECT_8), 93, "checkerboard under 8: ", covered=wr.covered_label)
    assert half.pixels == rows * cols // 2 and (half.x0, half.y0, half.x1, half.y1) == (0, 0, cols - 1, rows - 1)
    assert _check(ctx, board, wr.constant(0, 0, 0, 200, wr.WAND_GLOBAL), 94, "checkerboard, global: ", covered=wr.covered_label).pixels == rows * cols // 2


# ---- sub-image views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", roi_util.LAYOUTS_U8, ids=lambda l: f"lead{l[0]}_pitch+{l[1]}")
def test_sub_image_views(ctx, layout):
    """The three images inside larger allocations, odd lead bytes and pitches: nothing outside the views is written, nothing uncovered
    inside them, and the original not at all."""
    rows, cols = 37, 75
    lead, residue = layout
    rng = np.random.default_rng(100 + lead)
    for k, (flags, kind) in enumerate(((0, 1), (wr.WAND_CONNECT_8, 2))):
        orig = wr.quantised(rng, rows, cols)
        ed, scr = _pair_of(orig, 100 + k)
        wand = _kinds(70, 20, 12, flags, rows, cols)[kind]
        o, e, s = sub_views(orig, ed, scr, layout)
        info = ctx.fill_similar(wand, e.img, s.img, rows, cols, o.img)
        want = wr.fill_similar(wand, ed, scr, orig)
        assert np.array_equal(e.result(), ed) and np.array_equal(s.result(), scr), k
        o.assert_unchanged()
        assert (info.pixels, info.x0, info.y0, info.x1, info.y1) == want and 1 < info.pixels < rows * cols


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    orig = wr.quantised(np.random.default_rng(4), rows, cols)
    ed, scr = _pair_of(orig, 4)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    L = rt.lib()

    def W(**kw):
        f = dict(x=5, y=6, tolerance=12, flags=0, ax0=0, ay0=0, ax1=30, ay1=15, label0=3, label1=200); f.update(kw)
        return rt.Wand(*(f[k] for k in ("x", "y", "tolerance", "flags", "ax0", "ay0", "ax1", "ay1", "label0", "label1")))

    def call(wand=W(), edited=e.img, scribble=s.img, original=o.img, r=rows, c=cols, info=True):
        out = rt.WandInfo()
        return L.rtdd_fill_similar(ctx._h, C.byref(wand) if wand is not None else None, *raw_target(edited, scribble, original, r, c), C.byref(out) if info else None)

    refused = {
        "null wand": call(wand=None),
        "seed x < 0": call(W(x=-1)),
        "seed x == cols": call(W(x=cols)),
        "seed y < 0": call(W(y=-1)),
        "seed y == rows": call(W(y=rows)),
        "tolerance -1": call(W(tolerance=-1)),
        "tolerance 256": call(W(tolerance=256)),
        "flag 4": call(W(flags=4)),
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
        "painting without original": call(original=None),
        "erasing without original": call(W(label0=-1, label1=-1), original=None),
        "painting with a short original pitch": call(original=(o.img[0], cols * 3 - 1)),
        "null edited": call(edited=None),
        "null scribble": call(scribble=None),
        "negative rows": call(r=-1),
        "negative cols": call(c=-1),
        "no rows": call(W(x=0, y=0), r=0),
        "no cols": call(W(x=0, y=0), c=0),
        "edited pitch": call(edited=(e.img[0], cols * 3 - 1)),
        "scribble pitch": call(scribble=(s.img[0], cols - 1)),
        "rows above 32768": call(r=32769),
        "cols above 32768": call(c=32769, edited=(e.img[0], 1 << 20), scribble=(s.img[0], 1 << 20), original=(o.img[0], 1 << 20)),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    assert call() == 0 and call(info=False) == 0 and call(W(label0=-1, label1=-1)) == 0 and call(W(flags=3, tolerance=255)) == 0
    assert call(W(ax0=-32768, ay0=32767, ax1=32767, ay1=-32768, label0=255, label1=0, tolerance=0)) == 0
    with pytest.raises(rt.RtddError):
        ctx.fill_similar((5, 6, 12, 0, 0, 0, 1, 1, -1, 7), e.img, s.img, rows, cols, o.img)


# ---- on a pyramid --------------------------------------------------------------------------------------------------------------------------
_refs = {}


def _wands(bgr, ann, erasing):
    """Two painting selections, a constant one and a ramp down the image; erasing: also one that removes every label on pixels that look
    like a labelled one (global), that pixel included."""
    rows, cols = ann.shape
    out = [wr.constant(cols // 2, 10, 14, 3), (cols // 3, rows - 8, 14, wr.WAND_CONNECT_8, cols // 2, rows // 2, cols // 2, rows - 1, 200, 40)]
    if erasing:
        y, x = (int(v[0]) for v in np.nonzero(ann != 32))
        out.append(wr.erase(x, y, 30, wr.WAND_GLOBAL))
    return out


def _reference(oracle, lut, erasing):
    """The reduced pair: estimate, the wands (the erasing one only when asked for: then the rebuild), estimate."""
    if erasing not in _refs:
        bgr, ann = _pair()
        ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
        assert ref.P >= 3
        ref.estimate(ITERS)
        before = ref.scribble[0].copy()
        for wand in _wands(bgr, ann, erasing):
            wr.fill_similar(wand, ref.edited[0], ref.scribble[0], bgr, wr.covered_label)
        assert ((before != 255) & (ref.scribble[0] == 255)).sum() > 200
        if erasing:
            assert ((before == 255) & (ref.scribble[0] == 0)).sum() >= 1
            sr.rebuild(ref)                                           # the erasing call asks for the rebuild itself
        ref.estimate(ITERS)
        _refs[erasing] = ref
    return _refs[erasing]


@pytest.mark.parametrize("erasing", [False, True], ids=["painting", "erasing"])
def test_wands_on_the_pyramid_between_two_estimates(oracle, lut, erasing):
    """estimate queued, the wands, estimate again, with no synchronisation of the test's own between them"""
    bgr, ann = _pair()
    rows, cols = ann.shape
    ref = _reference(oracle, lut, erasing)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == ref.P
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS)
        sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
        for wand in _wands(bgr, ann, erasing):
            assert c.fill_similar(wand, (ep[0], ep[1]), (sp[0], sp[1]), rows, cols, (op[0], op[1])).pixels >= 1
        c.estimate_depth(ITERS); c.synchronize()
        _assert_pyramid(c, ref, "erasing" if erasing else "painting")
    if erasing:                                                       # not vacuous: without the rebuild the coarse levels keep the erased labels
        kept = _reference(oracle, lut, False)
        assert any((ref.scribble[l] != kept.scribble[l]).any() for l in range(1, ref.P))


def test_a_retired_live_pointer_is_refused():
    bgr, ann = _pair()
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann)); c.synchronize()
        old_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0); old_e = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
        wand = wr.constant(50, 11, 8, 64)
        c.fill_similar(wand, (old_e[0], old_e[1]), (old_s[0], old_s[1]), rows, cols, (op[0], op[1]))          # fine: still the pyramid's
        scr = rt.host_image((rows, cols)); ed = rt.host_image((rows, cols, 3)); out = rt.host_image((rows, cols))
        scr.a[...] = c.pyramid_download(rt.IMG_SCRIBBLE, 0); ed.a[...] = c.pyramid_download(rt.IMG_EDITED, 0)
        assert scr.a[11, 50] == 255 and (ed.a[11, 50] == 64).all()
        c.live_submit(scr.a, ed.a, out.a, 50); c.live_wait()
        with pytest.raises(rt.RtddError) as err:
            c.fill_similar(wand, (old_e[0], old_e[1]), (old_s[0], old_s[1]), rows, cols, (op[0], op[1]))
        assert err.value.status == 2
        new_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0); new_e = c.pyramid_image(rt.IMG_EDITED, 0)
        assert new_s[0] != old_s[0]
        c.fill_similar(wr.constant(50, 11, 8, 128), (new_e[0], new_e[1]), (new_s[0], new_s[1]), rows, cols, (op[0], op[1]))
        assert (c.pyramid_download(rt.IMG_EDITED, 0)[11, 50] == 128).all()
        for x in (scr, ed, out):
            x.free()


# ---- the scratch ---------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_is_shared_with_the_defocus_table():
    """A table-path defocus, a wand (its bit planes overwrite the table and its zero padding), the same defocus: equal outputs."""
    from gpu_util import down
    rows, cols = 120, 200
    rng = np.random.default_rng(9)
    orig = wr.quantised(rng, rows, cols)
    depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
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
                _check(c, orig, wr.constant(100, 60, 15, 200, wr.WAND_CONNECT_8), 110, "between the two defocus calls: ")
        assert np.array_equal(outs[0], outs[1])
