"""rtdd_fill_polygon on the GPU, through the C ABI (-m gpu): every comparison is byte equality of both images against
tests/polygon_ref.py (or, for whole estimates, of every level against the restated cascade fed with the restated annotation).  The shapes
are the smallest at which the kernel's tiles can go wrong: one 64 x 16 tile across with a ragged last row of tiles (67 x 45), three tiles
across so that an edge can lie left of, right of and across a tile (37 x 150), the vertex cap (768 edges: three culling passes), and
two-pixel-wide images as long as the domain for the arithmetic's width."""
import ctypes as C

import numpy as np
import pytest

import polygon_ref as pr
import ramp_ref as rr
import realtimedepthdiffusion_amd as rt
import roi_util
import strokes_ref as sr
from cascade_ref import Cascade
from gpu_util import up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _assert_pyramid, _Dev, _images, _pair, raw_target, sub_views

pytestmark = pytest.mark.gpu


def _start(rows, cols, seed):
    orig, ed, scr = _images(rows, cols, seed)
    scr[::3, ::4] = 255                                               # (so that an erasure shows in the scribble too)
    return orig, ed, scr


def _check(c, V, fill, rows, cols, seed, what=""):
    orig, ed, scr = _start(rows, cols, seed)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    c.fill_polygon(V, fill, e.img, s.img, rows, cols, original=o.img)
    c.synchronize()
    covered = pr.fill_polygon(V, fill, ed, scr, orig)
    got_e, got_s = e.host(), s.host()
    print(f"{what}{rows}x{cols}, {len(V)} vertices, fill {fill}: scribble differs at {int((got_s != scr).sum())}, edited at {int((got_e != ed).any(-1).sum())} pixels; {covered} covered")
    assert np.array_equal(got_s, scr) and np.array_equal(got_e, ed), what
    assert np.array_equal(o.host(), orig)
    return covered


# ---- one tile wide: 67 x 45 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [pr.FILL_NONZERO, pr.FILL_EVEN_ODD])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["constant", "ramp", "erase"])
def test_random_contours_one_tile_wide(ctx, rule, kind):
    rows, cols = 67, 45
    rng = np.random.default_rng(10 + 3 * rule + kind)
    covered = 0
    for i in range(16):
        V = pr.random_contour(rng, rows, cols, 1 + (5 * i + kind) % 12)
        covered += _check(ctx, V, pr.random_fill(rng, rows, cols, kind, rule), rows, cols, 20 + i)
    assert covered > 2000


def test_a_contour_round_the_whole_image_and_one_wholly_outside(ctx):
    rows, cols = 67, 45
    around = [(-5, -5), (60, -5), (60, 80), (-5, 80)]
    assert pr.fill_polygon_tiled(around, pr.constant(1), *_images(rows, cols, 0)[1:], None) == (5, 5, 0)        # every tile uniform and covered
    for fill in (pr.constant(77), (pr.FILL_EVEN_ODD, 3, -4, 40, 70, 5, 250), pr.erase()):
        assert _check(ctx, around, fill, rows, cols, 30) == rows * cols
        assert _check(ctx, around[::-1], fill, rows, cols, 30) == rows * cols
    for V in ([(-50, -5), (-3, -5), (-3, 80)], [(45, 0), (90, 20), (50, 66)], [(3, 67), (40, 70), (20, 90)], [(0, -1), (44, -1)], [(-1, -1)]):
        for fill in (pr.constant(77), pr.erase()):
            assert _check(ctx, V, fill, rows, cols, 31) == 0          # no write: _check compares with the untouched images, padding included


# ---- three tiles across: 37 x 150 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.BORDER_CONTOURS))
def test_tile_borders_and_edge_classes(ctx, name):
    rows, cols = 37, 150
    V = pr.BORDER_CONTOURS[name]
    for i, fill in enumerate((pr.constant(200), pr.constant(3, pr.FILL_EVEN_ODD), (pr.FILL_NONZERO, 3, 2, 140, 30, 250, 4), (pr.FILL_EVEN_ODD, 140, 35, 10, 0, 0, 255),
                              pr.erase(), pr.erase(pr.FILL_EVEN_ODD))):
        assert _check(ctx, V, fill, rows, cols, 40 + i, name + ": ") > 0


@pytest.mark.parametrize("rule", [pr.FILL_NONZERO, pr.FILL_EVEN_ODD])
def test_random_contours_three_tiles_wide(ctx, rule):
    rows, cols = 37, 150
    rng = np.random.default_rng(50 + rule)
    for i in range(18):
        V = pr.random_contour(rng, rows, cols, 1 + (7 * i) % 12, margin=70)
        _check(ctx, V, pr.random_fill(rng, rows, cols, i % 3, rule), rows, cols, 50 + i)


# ---- the vertex cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [pr.FILL_NONZERO, pr.FILL_EVEN_ODD])
def test_the_vertex_cap(ctx, rule):
    rows, cols = 150, 200
    ring = pr.spiky_ring(768, 100, 75, 30, 90)
    assert len(ring) == 768 and len(set(ring)) > 500
    assert 3000 < _check(ctx, ring, (rule, 0, 0, 199, 149, 10, 240), rows, cols, 60) < rows * cols
    twice = pr.spiky_ring(384, 100, 75, 60, 110) + pr.spiky_ring(384, 90, 70, 20, 50)      # two rings in one contour: they overlap, w reaches 2
    assert np.abs(pr.windings(twice, rows, cols)[2]).max() >= 2
    _check(ctx, twice, pr.constant(9, rule), rows, cols, 61)
    _check(ctx, twice, pr.erase(rule), rows, cols, 62)
    for V in ([(100, 75)], [(3, 140), (190, 7)], [(10, 10), (190, 20), (64, 140)], [(0, 0), (199, 149)], [(5, 5), (5, 5), (5, 5)]):
        assert _check(ctx, V, (rule, 0, 0, 199, 149, 10, 240), rows, cols, 63) >= 1


# ---- the arithmetic's width ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(2, 32768), (32768, 2)])
def test_contours_through_the_domains_corners(ctx, rows, cols):
    """cr passes 2^31 here and each of its two products 2^32; the axes' dd nears 2^35: a 32-bit slip shows."""
    some = 0
    for i, V in enumerate(pr.EXTREME_CONTOURS):
        ax = pr.EXTREME_AXES[i % len(pr.EXTREME_AXES)]
        some += _check(ctx, V, (i % 2, *ax, 0, 255), rows, cols, 70 + i)
        some += _check(ctx, V, (1 - i % 2, *ax, 255, 3), rows, cols, 70 + i)
    _check(ctx, pr.EXTREME_CONTOURS[3], pr.erase(), rows, cols, 79)
    assert some > 100000 and max(pr.max_abs_cr(V, rows, cols) for V in pr.EXTREME_CONTOURS) > 2 ** 31


def test_extreme_axes(ctx):
    rows, cols = 67, 45
    around = [(-5, -5), (60, -5), (60, 80), (-5, 80)]
    many = 0
    for i, q in enumerate(rr.extreme_strokes()):
        fill = (pr.FILL_NONZERO, q[0], q[1], q[2], q[3], q[6], q[7])
        assert _check(ctx, around, fill, rows, cols, 80 + i) == rows * cols
        ed = np.zeros((rows, cols, 3), np.uint8)
        pr.fill_polygon(around, fill, ed, np.zeros((rows, cols), np.uint8))
        many = max(many, len(np.unique(ed)))
    assert many > 40


# ---- sub-image views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", roi_util.LAYOUTS_U8, ids=lambda l: f"lead{l[0]}_pitch+{l[1]}")
def test_sub_image_views(ctx, layout):
    """The three images inside larger allocations, odd lead bytes and pitches: nothing outside the views is written, nothing uncovered
    inside them, and the original not at all."""
    rows, cols = 37, 75
    lead, residue = layout
    for k, (V, fill) in enumerate((([(5, 3), (70, 8), (80, 30), (30, 40), (-4, 20)], (pr.FILL_NONZERO, 0, 0, 74, 36, 20, 230)),
                                   (pr.scaled(pr.PENTAGRAM, 2, 1, -6, -5), pr.erase(pr.FILL_EVEN_ODD)))):
        orig, ed, scr = _start(rows, cols, 90 + lead)
        o, e, s = sub_views(orig, ed, scr, layout)
        ctx.fill_polygon(V, fill, e.img, s.img, rows, cols, original=o.img)
        ctx.synchronize()
        covered = pr.fill_polygon(V, fill, ed, scr, orig)
        assert np.array_equal(e.result(), ed) and np.array_equal(s.result(), scr), k
        o.assert_unchanged()
        assert 0 < covered < rows * cols                              # (some pixels the contour does not cover: they must keep their bytes)


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
def test_calls_compose_in_stream_order(ctx):
    rows, cols = 67, 150
    orig, ed, scr = _start(rows, cols, 100)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    first = [(5, 5, 140, 60, 9, sr.BRUSH_ROUND, 30, 220), (140, 5, 5, 60, 7, sr.BRUSH_SQUARE, 90, 90)]
    lasso = [(20, -5), (130, 10), (100, 70), (60, 30), (10, 66)]
    hole = [(50, 10), (110, 20), (90, 50), (60, 25)]
    last = [(0, 33, 149, 35, 5, sr.BRUSH_SQUARE, 250, 1), (75, 0, 75, 66, 3, sr.BRUSH_ROUND, sr.STROKE_ERASE, sr.STROKE_ERASE)]
    fill = (pr.FILL_NONZERO, 20, 0, 130, 66, 10, 200)
    ctx.paint_ramp_strokes(first, e.img, s.img, rows, cols, original=o.img)
    ctx.fill_polygon(lasso, fill, e.img, s.img, rows, cols)
    ctx.fill_polygon(hole, pr.erase(), e.img, s.img, rows, cols, original=o.img)
    ctx.paint_ramp_strokes(last, e.img, s.img, rows, cols, original=o.img)
    ctx.synchronize()
    rr.paint_ramp_strokes(first, ed, scr, orig)
    pr.fill_polygon(lasso, fill, ed, scr, orig)
    pr.fill_polygon(hole, pr.erase(), ed, scr, orig)
    rr.paint_ramp_strokes(last, ed, scr, orig)
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    other_e, other_s = _start(rows, cols, 100)[1:]                    # (the order matters here: the hole first gives other bytes)
    pr.fill_polygon(hole, pr.erase(), other_e, other_s, orig); pr.fill_polygon(lasso, fill, other_e, other_s, orig)
    rr.paint_ramp_strokes(first + last, other_e, other_s, orig)
    assert not np.array_equal(other_s, scr)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    orig, ed, scr = _images(rows, cols, 4)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    L = rt.lib()
    tri = ((5, 5), (25, 7), (12, 17))

    def F(**kw):
        f = dict(rule=0, ax0=0, ay0=0, ax1=30, ay1=15, label0=3, label1=200); f.update(kw)
        return rt.Fill(*(f[k] for k in ("rule", "ax0", "ay0", "ax1", "ay1", "label0", "label1")))

    def call(pts=tri, n=None, fill=F(), edited=e.img, scribble=s.img, original=o.img, r=rows, c=cols, null_xy=False):
        flat = [v for p in pts for v in p]
        xy = (C.c_int * max(len(flat), 2))(*flat)
        return L.rtdd_fill_polygon(ctx._h, None if null_xy else xy, C.c_int(len(pts) if n is None else n), C.byref(fill) if fill is not None else None,
                                   *raw_target(edited, scribble, original, r, c))

    gone = F(label0=-1, label1=-1)
    refused = {
        "null fill": call(fill=None),
        "null xy with n > 0": call(null_xy=True, n=3),
        "n < 0": call(n=-1),
        "n > 768": call(pts=[(1, 1)] * 769),
        "rule 2": call(fill=F(rule=2)),
        "rule -1": call(fill=F(rule=-1)),
        "vertex x too small": call(pts=((-32769, 0), (1, 1), (2, 9))),
        "vertex x too large": call(pts=((0, 0), (32768, 1), (2, 9))),
        "vertex y too small": call(pts=((0, 0), (1, -32769), (2, 9))),
        "vertex y too large": call(pts=((0, 0), (1, 1), (2, 32768))),
        "ax0 too small": call(fill=F(ax0=-32769)),
        "ay0 too large": call(fill=F(ay0=32768)),
        "ax1 too large": call(fill=F(ax1=32768)),
        "ay1 too small": call(fill=F(ay1=-32769)),
        "an axis outside the domain under equal labels": call(fill=F(ax1=40000, label1=3)),
        "label0 256": call(fill=F(label0=256)),
        "label1 256": call(fill=F(label1=256)),
        "label0 -2": call(fill=F(label0=-2)),
        "label1 -2": call(fill=F(label1=-2)),
        "only label0 erases": call(fill=F(label0=-1)),
        "only label1 erases": call(fill=F(label1=-1)),
        "erase without original": call(fill=gone, original=None),
        "erase with a short original pitch": call(fill=gone, original=(o.img[0], cols * 3 - 1)),
        "null edited": call(edited=None),
        "null scribble": call(scribble=None),
        "negative rows": call(r=-1),
        "negative cols": call(c=-1),
        "edited pitch": call(edited=(e.img[0], cols * 3 - 1)),
        "scribble pitch": call(scribble=(s.img[0], cols - 1)),
        "rows above 32768": call(r=32769),
        "cols above 32768": call(c=32769, edited=(e.img[0], 1 << 20), scribble=(s.img[0], 1 << 20)),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    # n == 0 is OK and writes nothing, with or without an array
    assert call(n=0) == 0 and call(null_xy=True, n=0) == 0 and call(n=0, fill=gone) == 0
    ctx.synchronize()
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    assert call() == 0 and call(original=None) == 0 and call(fill=gone) == 0 and call(pts=[(i % 30, i % 17) for i in range(768)]) == 0
    assert call(pts=((-32768, 32767), (32767, -32768), (5, 5)), fill=F(ax0=-32768, ay0=32767, ax1=32767, ay1=-32768, label0=255, label1=0)) == 0
    ctx.synchronize()
    with pytest.raises(rt.RtddError):
        ctx.fill_polygon(tri, (0, 0, 0, 1, 1, -1, 7), e.img, s.img, rows, cols, original=o.img)


# ---- on a pyramid --------------------------------------------------------------------------------------------------------------------------
_refs = {}


def _lassos(ann):
    """A floor filled with a ramp over the labels' lower half, a constant region at the top, and an erasing lasso across the labels."""
    rows, cols = ann.shape
    y = int(np.median(np.nonzero(ann != 32)[0]))
    floor = ([(cols // 3, rows // 2), (2 * cols // 3, rows // 2), (cols + 20, rows + 5), (-20, rows + 5)], (pr.FILL_NONZERO, cols // 2, rows // 2, cols // 2, rows - 1, 200, 40))
    sky = ([(10, 5), (cols - 10, 8), (cols // 2, 50)], pr.constant(3))
    gone = ([(-5, y - 30), (cols // 2, y - 10), (cols + 5, y - 30), (cols + 5, y + 30), (cols // 2, y + 10), (-5, y + 30)], pr.erase())
    return floor, sky, gone


def _reference(oracle, lut, erasing):
    """The reduced pair: estimate, the lassos (the erasing one only when asked for: then the rebuild), estimate."""
    if erasing not in _refs:
        bgr, ann = _pair()
        ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
        assert ref.P >= 3
        ref.estimate(ITERS)
        before = ref.scribble[0].copy()
        floor, sky, gone = _lassos(ann)
        for V, fill in (floor, sky) + ((gone,) if erasing else ()):
            pr.fill_polygon(V, fill, ref.edited[0], ref.scribble[0], bgr)
        assert ((before != 255) & (ref.scribble[0] == 255)).sum() > 2000 and len(np.unique(ref.edited[0][ref.scribble[0] == 255])) > 100
        if erasing:
            assert ((before == 255) & (ref.scribble[0] == 0)).sum() > 200
            sr.rebuild(ref)                                           # the erasing call asks for the rebuild itself
        ref.estimate(ITERS)
        _refs[erasing] = ref
    return _refs[erasing]


@pytest.mark.parametrize("erasing", [False, True], ids=["painting", "erasing"])
def test_fills_on_the_pyramid_then_an_estimate(oracle, lut, erasing):
    bgr, ann = _pair()
    rows, cols = ann.shape
    ref = _reference(oracle, lut, erasing)
    floor, sky, gone = _lassos(ann)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        assert c.pyramid_create(rows, cols) == ref.P
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS)
        sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
        for V, fill in (floor, sky) + ((gone,) if erasing else ()):
            c.fill_polygon(V, fill, (ep[0], ep[1]), (sp[0], sp[1]), rows, cols, original=(op[0], op[1]))
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
        old_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0); old_e = c.pyramid_image(rt.IMG_EDITED, 0)
        tri = [(5, 5), (100, 9), (50, 90)]
        c.fill_polygon(tri, pr.constant(64), (old_e[0], old_e[1]), (old_s[0], old_s[1]), rows, cols)          # fine: still the pyramid's
        scr = rt.host_image((rows, cols)); ed = rt.host_image((rows, cols, 3)); out = rt.host_image((rows, cols))
        scr.a[...] = c.pyramid_download(rt.IMG_SCRIBBLE, 0); ed.a[...] = c.pyramid_download(rt.IMG_EDITED, 0)
        assert (scr.a[10:13, 50] == 255).all()
        c.live_submit(scr.a, ed.a, out.a, 50); c.live_wait()
        with pytest.raises(rt.RtddError) as err:
            c.fill_polygon(tri, pr.constant(128), (old_e[0], old_e[1]), (old_s[0], old_s[1]), rows, cols)
        assert err.value.status == 2
        new_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0); new_e = c.pyramid_image(rt.IMG_EDITED, 0)
        assert new_s[0] != old_s[0]
        c.fill_polygon(tri, pr.constant(128), (new_e[0], new_e[1]), (new_s[0], new_s[1]), rows, cols)
        c.synchronize()
        assert (c.pyramid_download(rt.IMG_EDITED, 0)[10, 50] == 128).all()
        for x in (scr, ed, out):
            x.free()
