"""rtdd_segment_surfaces on the GPU, through the C ABI (-m gpu): every comparison is byte equality against tests/segment_ref.py -- both
images with their padding, the label map with its padding, the inputs unchanged, the info and every record.  The shapes are the wands':
one ragged word across and five tiles down (67 x 45), four words by ten tiles (150 x 200), three words by three tiles (37 x 150), and a
two-pixel-wide image 2000 rows long: one component through 125 tiles.  The fields of 67 x 45 have up to 2524 components: more than
SEGMENT_HEAD candidates, so that the second read-back runs, and fewer."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import regions_ref as rr
import remove_ref as rmr
import roi_util
import segment_ref as sg
import surface_ref as sf
import wand_ref as wr
from gpu_util import down, up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _Dev, _pair, sub_views
from segment_ref import ranking_map, rings, scene, six_fields, u_shape

pytestmark = pytest.mark.gpu
f32 = np.float32
STALE = 0x5A5A5A5A                                                    # what a label map holds before the call
OPTIONS = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, True)]      # labels, pair, records


def _pair_of(rows, cols, seed):
    """An edited image and a scribble image with labels in them."""
    rng = np.random.default_rng(seed)
    ed = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    scr = np.zeros((rows, cols), np.uint8)
    scr[::3, ::4] = 255
    return ed, scr


def _call(c, s, edited, scribble, depth, labels, rows, cols, records=True, info=True):
    """the raw ABI: (status, info, records or None); an image is (pointer, pitch) or None"""
    g = s if isinstance(s, rt.Segmentation) or s is None else rt.Segmentation(*s)
    out, arr = rt.SegmentInfo(), (rt.Segment * 256)()
    for r in arr:
        r.code = -7
    img = lambda t: (C.c_void_p(t[0]), C.c_size_t(t[1])) if t else (None, C.c_size_t(0))
    rc = rt.lib().rtdd_segment_surfaces(c._h, C.byref(g) if g is not None else None, *img(edited), *img(scribble), *img(depth), *img(labels), C.c_int(rows),
                                        C.c_int(cols), arr if records else None, C.byref(out) if info else None)
    filled = [k for k in range(256) if arr[k].code != -7]
    if rc != 0 or not records:
        assert filled == [], "records were written"
    elif info:
        assert filled == list(range(out.regions)), "records beyond the regions were written"
    return rc, sg.info_of(out), [sg.record_of(arr[k]) for k in filled] if records else None


def _check(c, depth, s, seed=0, what="", labels=True, pair=True, records=True, ref=sg.labels_graph):
    rows, cols = depth.shape
    ed, scr = _pair_of(rows, cols, seed)
    lab0 = np.full((rows, cols), STALE, np.int32)
    e, sc, d, l = _Dev(ed), _Dev(scr), _Dev(depth.view(np.uint8)), _Dev(lab0.view(np.uint8))
    rc, info, rec = _call(c, s, e.img if pair else None, sc.img if pair else None, d.img, l.img if labels else None, rows, cols, records)
    assert rc == 0, (what, rc)
    c.synchronize()                                                   # (the paint pass is queued behind the call's own synchronisation)
    want_lab, want_info, want_rec = sg.segment_surfaces(s, ed if pair else None, scr if pair else None, depth, ref)
    got_lab = l.host().view(np.int32)
    print(f"{what}{rows}x{cols}, {s}: info {info} against {want_info}; labels differ at {int((got_lab != (want_lab if labels else lab0)).sum())} pixels")
    assert info == want_info, what
    assert np.array_equal(got_lab, want_lab if labels else lab0), what
    assert np.array_equal(sc.host(), scr) and np.array_equal(e.host(), ed), what
    assert np.array_equal(d.host(), depth.view(np.uint8)), "the depth map was written"
    if records:
        assert rec == want_rec, what
    return want_lab, info, rec


# ---- random fields ---------------------------------------------------------------------------------------------------------------------------
def test_random_fields_one_word_wide(ctx):
    candidates = []
    bands = [(0, 255), (101, 106), (0, 255), (103, 103), (0, 255), (102.5, 255)]
    limits = [(1, 255), (3, 20), (1, 3), (1, 255), (2, 255), (1, 1)]
    for i, (step, depth) in enumerate(six_fields()):
        for j, (labels, pair, records) in enumerate(OPTIONS):
            lo, hi = bands[(i + j) % 6]
            mn, mx = limits[(i + 2 * j) % 6]
            s = sg.seg(step, lo, hi, mn, mx, 1 + (256 - mx) // 2 * (j % 2))
            _, info, _ = _check(ctx, depth, s, 10 * i + j, f"field {i}.{j}: ", labels, pair, records)
            candidates.append(info[1])
    assert max(candidates) > sg.HEAD and min(candidates) <= 4 and sum(1 < n <= sg.HEAD for n in candidates) > 5     # both read-back paths ran
    lab, info, rec = _check(ctx, six_fields()[0][1], sg.seg(0), 99, "step 0, everything: ")
    assert info[:3] == (2524, 2524, 255) and [r[1] for r in rec[:5]] == [7, 6, 6, 6, 5]


def test_random_fields_with_word_and_tile_borders(ctx):
    rows, cols = 150, 200
    rng = np.random.default_rng(30)
    for i, step in enumerate(sf.STEPS):
        lo, hi = ((0, 255), (101, 107))[i % 2]
        labels, pair, records = OPTIONS[i % 5]
        _check(ctx, sf.field(rng, rows, cols), sg.seg(step, lo, hi, 1 + i, 255 - 40 * i, 1 + 8 * i), 30 + i, f"borders {i}: ", labels, pair, records)
    _check(ctx, sf.field(rng, 37, 150), sg.seg(2.5, min_pixels=4), 37, "three words, three tiles: ")


def test_the_python_wrapper_and_the_use_case(ctx):
    depth, obj, box = scene()
    rows, cols = depth.shape
    ed, scr = _pair_of(rows, cols, 5)
    e, sc, d = _Dev(ed), _Dev(scr), _Dev(depth.view(np.uint8))
    l = _Dev(np.full((rows, cols), STALE, np.int32).view(np.uint8))
    s = sg.seg(4, min_pixels=16)
    info, rec = ctx.segment_surfaces(s, e.img, sc.img, rows, cols, d.img, l.img)
    ctx.synchronize()
    lab, want_info, want_rec = sg.segment_surfaces(s, ed, scr, depth)
    assert sg.info_of(info) == want_info and [sg.record_of(r) for r in rec] == want_rec and info.regions == 3
    assert np.array_equal(e.host(), ed) and np.array_equal(sc.host(), scr) and np.array_equal(l.host().view(np.int32), lab)
    info, rec = ctx.segment_surfaces(rt.Segmentation(*s), None, None, rows, cols, d.img)       # the records alone
    assert sg.info_of(info) == want_info and [sg.record_of(r) for r in rec] == want_rec
    with pytest.raises(rt.RtddError):
        ctx.segment_surfaces(sg.seg(4, first_code=251, max_regions=6), e.img, sc.img, rows, cols, d.img)


# ---- union-find traps --------------------------------------------------------------------------------------------------------------------------
def test_a_spiral_and_the_four_combs(ctx):
    rows, cols = 150, 200
    for k, mask in enumerate([wr.spiral(rows, cols)] + [wr.comb(rows, cols, d) for d in ("left", "right", "up", "down")] + [wr.comb(37, 150, "down")]):
        lab, info, rec = _check(ctx, sf.from_mask(mask), sg.seg(4), 50 + k, f"trap {k}: ")
        assert np.array_equal(lab == lab[mask].min(), mask) and mask.sum() in [r[1] for r in rec]
        _check(ctx, sf.from_mask(mask), sg.seg(4, 0, 100, max_regions=9, first_code=9), 60 + k, f"trap {k}, the mask alone: ")


def test_a_u_whose_arms_meet_in_the_tile_below(ctx):
    m = u_shape()
    lab, info, rec = _check(ctx, sf.from_mask(m), sg.seg(4, 0, 100), 70, "U: ")
    assert info == (1, 1, 1, int(m.sum())) and (rec[0][2], rec[0][3]) == (5, 2)
    big = np.zeros((100, 300), bool)                                  # ... and with the arms in different words, meeting three tiles down
    big[1:60, 3] = big[1:60, 290] = big[59, 3:291] = True
    lab, info, rec = _check(ctx, sf.from_mask(big), sg.seg(4, 0, 100), 71, "wide U: ")
    assert info == (1, 1, 1, int(big.sum()))


def test_concentric_rings_stay_distinct(ctx):
    d = rings()
    lab, info, rec = _check(ctx, d, sg.seg(4), 72, "rings: ")
    assert info[0] == 8 and len({r[8] for r in rec}) == 8
    assert _check(ctx, d, sg.seg(10), 73, "rings, one step wider: ")[1][:3] == (1, 1, 1)


def test_a_long_vertical_path(ctx):
    """test_gpu_fill_surface's 2000 x 2: a ramp of 0.1 per row down the left column, a wall down the right one, round the corner at the bottom"""
    rows, cols = 2000, 2
    depth = np.empty((rows, cols), f32)
    depth[:, 0] = (np.arange(rows) * 0.1).astype(f32)
    depth[:, 1] = 250
    depth[-1, 1] = depth[-1, 0]
    lab, info, rec = _check(ctx, depth, sg.seg(0.125), 90, "long: ")
    assert info == (2, 2, 2, 2 * rows) and rec[0][:8] == (1, rows + 1, 0, 0, 0, 0, 1, rows - 1) and rec[1][:4] == (2, rows - 1, 1, 0)


def test_links_are_not_a_property_of_one_pixel(ctx):
    yy, xx = np.mgrid[:20, :30]
    board = np.where((yy + xx) & 1, f32(104), f32(100)).astype(f32)
    lab, info, rec = _check(ctx, board, sg.seg(3), 100, "checkerboard, step 3: ")
    assert info == (600, 600, 255, 255) and [r[3] * 30 + r[2] for r in rec] == list(range(255))
    assert _check(ctx, board, sg.seg(4), 101, "checkerboard, step 4: ")[1] == (1, 1, 1, 600)
    col = np.mgrid[:10, :70][1]
    assert _check(ctx, (f32(2) * col).astype(f32), sg.seg(2, 60, 80), 102, "slope 2: ")[1] == (1, 1, 1, 110)
    assert _check(ctx, (f32(2.5) * col).astype(f32), sg.seg(2), 103, "slope 2.5: ")[1] == (70, 70, 70, 700)
    stairs = (f32(50) + f32(5) * (np.mgrid[:12, :60][1] // 10)).astype(f32)
    lab, info, rec = _check(ctx, stairs, sg.seg(3), 104, "terraces: ")
    assert info == (6, 6, 6, 720) and [(r[4], r[6]) for r in rec] == [(10 * k, 10 * k + 9) for k in range(6)]
    depth, order = ranking_map()
    lab, info, rec = _check(ctx, depth, sg.seg(1, 0, 150), 105, "ranking: ")
    assert [r[3] * 11 + r[2] for r in rec] == order
    assert _check(ctx, depth, sg.seg(1, 0, 150, 3, 4, 250), 106, "ranking, cut: ")[1] == (10, 5, 4, 14)


def test_exact_thresholds(ctx):
    row = np.array([[100, 103, np.nextafter(f32(106), f32(np.inf)), 50]], f32)
    lab, info, _ = _check(ctx, row, sg.seg(3), 110, "step: ")
    assert lab.tolist() == [[0, 0, 2, 3]]
    lo, hi = f32(100) - f32(7), f32(100) + f32(9)
    below, above = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
    edge = np.array([[below, lo, 100, hi, above]], f32)
    assert _check(ctx, edge, sg.seg(255, float(lo), float(hi)), 111, "band: ")[0].tolist() == [[-1, 1, 1, 1, -1]]
    assert _check(ctx, edge, sg.seg(255, float(below), float(above)), 112, "band, one ulp wider: ")[0].tolist() == [[0, 0, 0, 0, 0]]
    assert _check(ctx, edge, sg.seg(255, float(np.nextafter(lo, f32(np.inf))), float(np.nextafter(hi, f32(-np.inf)))), 113,
                  "band, one ulp narrower: ")[0].tolist() == [[-1, -1, 2, -1, -1]]
    assert _check(ctx, edge, sg.seg(0, float(hi), float(hi)), 114, "lo == hi: ")[0].tolist() == [[-1, -1, -1, 3, -1]]


def test_special_values(ctx):
    rows, cols = 30, 70
    depth = sf.special_field(np.random.default_rng(7), rows, cols)
    lab, info, rec = _check(ctx, depth, sg.seg(0, 0, 0), 120, "zeros: ")
    assert (lab[5, 3:8] == lab[5, 3]).all() and lab[5, 3] >= 0 and lab[6, 5] == -1 and np.array_equal(lab >= 0, sf.clamped(depth) == 0)
    assert all(r[8] == r[9] == 0 for r in rec)                        # NaN, -0 and the negatives are +0, bit for bit
    for k, s in enumerate((sg.seg(255), sg.seg(2.5), sg.seg(100, 1e-40, 255), sg.seg(0, 255, 255))):
        _check(ctx, depth, s, 121 + k, "special: ")


# ---- the wand, on the device ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["field", "spiral"])
def test_a_region_is_what_the_wand_covers_from_its_root(ctx, what):
    if what == "field":
        depth, s = six_fields()[2][1], sg.seg(2.5, min_pixels=5, max_regions=12, first_code=40)
    else:
        depth, s = sf.from_mask(wr.spiral(150, 200)), sg.seg(4, max_regions=4, first_code=7)
    rows, cols = depth.shape
    ed, scr = _pair_of(rows, cols, 3)
    d = _Dev(depth.view(np.uint8))
    e1, s1, e2, s2 = _Dev(ed), _Dev(scr), _Dev(ed), _Dev(scr)
    info, rec = ctx.segment_surfaces(s, e1.img, s1.img, rows, cols, d.img)
    assert info.regions >= (5 if what == "field" else 2)
    for r in rec:
        w = ctx.fill_surface(sf.constant(r.rootX, r.rootY, s[0], r.code), e2.img, s2.img, rows, cols, d.img)
        assert (w.pixels, w.x0, w.y0, w.x1, w.y1) == (r.pixels, r.x0, r.y0, r.x1, r.y1)
    ctx.synchronize()
    assert np.array_equal(e1.host(), e2.host()) and np.array_equal(s1.host(), s2.host())
    assert not np.array_equal(s1.host(), scr)


# ---- views and leftovers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(roi_util.LAYOUTS_U8)), ids=lambda k: f"u8{roi_util.LAYOUTS_U8[k]}_f32{roi_util.LAYOUTS_F32[k]}")
def test_sub_image_views(ctx, k):
    rows, cols = 37, 75
    layout, (dlead, dres) = roi_util.LAYOUTS_U8[k], roi_util.LAYOUTS_F32[k]
    llead, lres = roi_util.LAYOUTS_F32[(k + 3) % len(roi_util.LAYOUTS_F32)]
    depth = sf.field(np.random.default_rng(100 + k), rows, cols)
    ed, scr = _pair_of(rows, cols, 100 + k)
    _, e, sc = sub_views(np.zeros((rows, cols, 3), np.uint8), ed, scr, layout)
    d = roi_util.Roi(depth, dlead, roi_util.pitch_for(cols * 4, dlead, dres), roi_util.FILL_INPUT, what="depth")
    l = roi_util.Roi(np.full((rows, cols), STALE, np.int32).view(f32), llead, roi_util.pitch_for(cols * 4, llead, lres), roi_util.FILL_OUTPUT, seed=3, what="labels")
    s = sg.seg(2.5, 101, 107, 3, 30, 5)
    rc, info, rec = _call(ctx, s, e.img, sc.img, d.img, l.img, rows, cols)
    ctx.synchronize()
    lab, want_info, want_rec = sg.segment_surfaces(s, ed, scr, depth)
    assert rc == 0 and info == want_info and rec == want_rec and info[2] == 30 and (lab == -1).any()
    assert np.array_equal(e.result(), ed) and np.array_equal(sc.result(), scr) and np.array_equal(l.result().view(np.int32), lab)
    d.assert_unchanged()


def test_a_smaller_image_after_a_larger_one(ctx):
    rng = np.random.default_rng(8)
    _check(ctx, sf.field(rng, 150, 200), sg.seg(1), 130, "large: ")
    _check(ctx, sf.field(rng, 20, 33), sg.seg(1), 131, "small after large: ")
    _check(ctx, sf.field(rng, 67, 45), sg.seg(3.5, min_pixels=2), 132, "medium after small: ")


def test_the_scratch_is_shared_with_the_defocus_table():
    """A table-path defocus, a segmentation (its planes and parents overwrite the table and its zero padding), the same defocus: equal outputs."""
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
                _check(c, sf.field(rng, rows, cols), sg.seg(2.5), 110, "between the two defocus calls: ")
        assert np.array_equal(outs[0], outs[1])


def test_on_the_region_pair_behind_an_estimate_then_codes_then_removed():
    bgr, ann = _pair()
    rows, cols = ann.shape
    s = sg.seg(2.0, 0, 255, 200, 6, 3)
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
            e, m, k = c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], c.pyramid_image(rt.IMG_REGION_CODE)[:2]
            o, d = c.pyramid_image(rt.IMG_ORIGINAL)[:2], c.pyramid_image(rt.IMG_DEPTH)[:2]
            info, rec = c.segment_surfaces(s, e, m, rows, cols, d)
            c.region_codes(e, m, rows, cols, 0, k)
            art, z = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), f32))
            c.remove_object(o, d, k, art, z, rows, cols, rt.Removal(**rmr.removal(rec[min(1, len(rec) - 1)].code, 2, 0.0)))
            c.synchronize()
            got.append((c.pyramid_download(rt.IMG_DEPTH, 0), c.pyramid_download(rt.IMG_REGION_EDITED), c.pyramid_download(rt.IMG_REGION_MASK), down(art), down(z),
                        sg.info_of(info), [sg.record_of(r) for r in rec]))
    a, b = got
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:5], b[:5])) and a[5:] == b[5:]
    depth = a[0]
    ed, mask = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
    lab, want_info, want_rec = sg.segment_surfaces(s, ed, mask, depth)
    assert a[5] == want_info and a[6] == want_rec and want_info[2] >= 1
    assert np.array_equal(a[1], ed) and np.array_equal(a[2], mask)
    codes = rr.region_codes(ed, mask, 0)
    art, z = rmr.remove(bgr, depth, codes, rmr.removal(want_rec[min(1, len(want_rec) - 1)][0], 2, 0.0))
    assert np.array_equal(a[3], art) and rmr.same_bits(a[4], z) and not np.array_equal(art, bgr)


def test_a_retired_live_pointer_is_refused():
    bgr, ann = _pair()
    rows, cols = ann.shape
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann)); c.synchronize()
        old_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0)[:2]; old_e = c.pyramid_image(rt.IMG_EDITED, 0)[:2]; dp = c.pyramid_image(rt.IMG_DEPTH, 0)[:2]
        s = sg.seg(0, min_pixels=rows * cols, max_regions=1, first_code=64)
        assert c.segment_surfaces(s, old_e, old_s, rows, cols, dp)[0].regions <= 1       # fine: still the pyramid's
        scr = rt.host_image((rows, cols)); ed = rt.host_image((rows, cols, 3)); out = rt.host_image((rows, cols))
        scr.a[...] = c.pyramid_download(rt.IMG_SCRIBBLE, 0); ed.a[...] = c.pyramid_download(rt.IMG_EDITED, 0)
        c.live_submit(scr.a, ed.a, out.a, 50); c.live_wait()
        with pytest.raises(rt.RtddError) as err:
            c.segment_surfaces(s, old_e, old_s, rows, cols, dp)
        assert err.value.status == 2
        c.segment_surfaces(s, None, None, rows, cols, dp)             # without a pair there is nothing retired to write
        new_s = c.pyramid_image(rt.IMG_SCRIBBLE, 0)[:2]; new_e = c.pyramid_image(rt.IMG_EDITED, 0)[:2]
        assert new_s[0] != old_s[0]
        c.segment_surfaces(s, new_e, new_s, rows, cols, dp)
        for x in (scr, ed, out):
            x.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    depth = sf.field(np.random.default_rng(4), rows, cols)
    ed, scr = _pair_of(rows, cols, 4)
    lab0 = np.full((rows, cols), STALE, np.int32)
    e, s, d, l = _Dev(ed), _Dev(scr), _Dev(depth.view(np.uint8)), _Dev(lab0.view(np.uint8))
    names = [n for n, _ in rt.Segmentation._fields_]

    def G(**kw):
        f = dict(step=2.5, lo=0.0, hi=255.0, minPixels=2, maxRegions=10, firstCode=3, flags=0); f.update(kw)
        return rt.Segmentation(*(f[k] for k in names))

    def call(g=G(), edited=e.img, scribble=s.img, dep=d.img, labels=l.img, r=rows, c=cols, records=True, info=True):
        return _call(ctx, g, edited, scribble, dep, labels, r, c, records, info)[0]

    nan, inf = float("nan"), float("inf")
    big = (1 << 20)
    refused = {
        "null struct": call(g=None),
        "null depth": call(dep=None),
        "depth pitch below a row": call(dep=(d.img[0], cols * 4 - 4)),
        "depth pitch no multiple of 4": call(dep=(d.img[0], d.img[1] + 2)),
        "depth pointer at 2": call(dep=(d.img[0] + 2, d.img[1])),
        "depth pointer at 1": call(dep=(d.img[0] + 1, d.img[1])),
        "step NaN": call(G(step=nan)), "step inf": call(G(step=inf)), "step < 0": call(G(step=-0.5)), "step > 255": call(G(step=255.5)),
        "lo NaN": call(G(lo=nan)), "lo -inf": call(G(lo=-inf)), "lo < 0": call(G(lo=-1.0)), "lo > 255": call(G(lo=256.0, hi=256.0)),
        "hi NaN": call(G(hi=nan)), "hi inf": call(G(hi=inf)), "hi < 0": call(G(hi=-1.0)), "hi > 255": call(G(hi=256.0)),
        "lo > hi": call(G(lo=100.0, hi=99.5)),
        "minPixels 0": call(G(minPixels=0)), "minPixels -1": call(G(minPixels=-1)),
        "maxRegions 0": call(G(maxRegions=0)), "maxRegions 256": call(G(maxRegions=256, firstCode=1)), "maxRegions -1": call(G(maxRegions=-1)),
        "firstCode 0": call(G(firstCode=0)), "firstCode 256": call(G(firstCode=256, maxRegions=1)), "firstCode -1": call(G(firstCode=-1)),
        "firstCode 251 with 6 regions": call(G(firstCode=251, maxRegions=6)),
        "firstCode 2 with 255 regions": call(G(firstCode=2, maxRegions=255)),
        "flag 1": call(G(flags=1)), "flag -1": call(G(flags=-1)), "flag 2": call(G(flags=2)),
        "no rows": call(r=0), "no cols": call(c=0), "negative rows": call(r=-1), "negative cols": call(c=-1),
        "rows above 32768": call(r=32769),
        "cols above 32768": call(c=32769, edited=(e.img[0], big), scribble=(s.img[0], big), dep=(d.img[0], big), labels=(l.img[0], big)),
        "edited without scribble": call(scribble=None),
        "scribble without edited": call(edited=None),
        "edited pitch": call(edited=(e.img[0], cols * 3 - 1)),
        "scribble pitch": call(scribble=(s.img[0], cols - 1)),
        "labels pitch below a row": call(labels=(l.img[0], cols * 4 - 4)),
        "labels pitch no multiple of 4": call(labels=(l.img[0], l.img[1] + 2)),
        "labels pointer at 2": call(labels=(l.img[0] + 2, l.img[1])),
        "labels pointer at 1": call(labels=(l.img[0] + 1, l.img[1])),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr) and np.array_equal(d.host(), depth.view(np.uint8))
    assert np.array_equal(l.host().view(np.int32), lab0)
    assert ctx.get_option(rt.OPT_PENDING_CALLS) == 0
    assert call() == 0 and call(info=False) == 0 and call(records=False, info=False) == 0 and call(labels=None) == 0 and call(edited=None, scribble=None) == 0
    assert call(G(firstCode=250, maxRegions=6)) == 0 and call(G(firstCode=1, maxRegions=255)) == 0 and call(G(firstCode=255, maxRegions=1)) == 0
    assert call(G(step=0.0, lo=0.0, hi=0.0)) == 0 and call(G(step=255.0, lo=255.0, hi=255.0, minPixels=rows * cols + 1)) == 0
    assert ctx.get_option(rt.OPT_PENDING_CALLS) == 0
