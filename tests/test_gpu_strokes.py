"""rtdd_paint_strokes and rtdd_pyramid_annotation_rebuild on the GPU, through the C ABI, against tests/strokes_ref.py and the restated
cascade (-m gpu).  Images are pitched, their rows padded; the padding must stay as it was."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import strokes_ref as sr
from cascade_ref import Cascade
from gpu_util import assert_bit_equal, up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _assert_pyramid, _Dev, _images, _pair, _polyline, raw_target

pytestmark = pytest.mark.gpu


def _run(c, strokes, e, s, o, rows, cols):
    c.paint_strokes(strokes, e.img, s.img, rows, cols, original=o.img if o is not None else None)
    c.synchronize()


@pytest.mark.parametrize("rows,cols,n,seed", [(1, 1, 1, 1), (1, 1, 64, 2), (1, 300, 2, 3), (1, 300, 300, 4), (67, 45, 1, 5), (67, 45, 64, 6), (67, 45, 4096, 7),
                                              (1080, 1920, 2, 8), (1080, 1920, 300, 9), (1080, 1920, 4096, 10), (4320, 7680, 300, 11)])
def test_polylines_match_the_restatement(ctx, rows, cols, n, seed):
    orig, ed, scr = _images(rows, cols, seed)
    strokes = _polyline(np.random.default_rng(seed), rows, cols, n)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    _run(ctx, strokes, e, s, o, rows, cols)
    sr.paint_strokes(strokes, ed, scr, orig)
    got_e, got_s = e.host(), s.host()
    print(f"{rows}x{cols}, {n} strokes: scribble differs at {int((got_s != scr).sum())}, edited at {int((got_e != ed).any(-1).sum())} pixels; "
          f"{int((scr == 255).sum())} labelled")
    assert np.array_equal(got_s, scr) and np.array_equal(got_e, ed)
    assert np.array_equal(o.host(), orig)
    if n >= 64 and rows * cols > 1:                                  # the order matters in these cases: backwards gives other pixels
        e2, s2 = orig.copy(), np.zeros((rows, cols), np.uint8)
        sr.paint_strokes(strokes[::-1], e2, s2, orig)
        assert not (np.array_equal(e2, ed) and np.array_equal(s2, scr))


@pytest.mark.parametrize("brush", [sr.BRUSH_SQUARE, sr.BRUSH_ROUND])
def test_single_stamps_and_strokes_wholly_outside(ctx, brush):
    rows, cols = 67, 45
    for i, (x, y, radius) in enumerate([(0, 0, 0), (22, 33, 1), (22, 33, 25), (44, 66, 11), (-3, 70, 9), (45, 67, 2), (10, 10, 1024), (-600, 5, 1024),
                                        (200, 200, 31), (-20, -20, 39), (-20, -20, 41)]):
        orig, ed, scr = _images(rows, cols, 100 + i)
        o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
        q = [(x, y, x, y, radius, brush, 200 - i)]
        _run(ctx, q, e, s, None, rows, cols)
        sr.paint_strokes(q, ed, scr)
        assert np.array_equal(s.host(), scr) and np.array_equal(e.host(), ed), q
    outside = [(-300, -300, -100, -250, 64, brush, 5), (cols + 40, 3, cols + 90, 60, 70, brush, sr.STROKE_ERASE), (3, rows + 17, 40, rows + 17, 32, brush, 9)]
    orig, ed, scr = _images(rows, cols, 1)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    _run(ctx, outside, e, s, o, rows, cols)
    assert np.array_equal(s.host(), scr) and np.array_equal(e.host(), ed)


def test_no_strokes_is_ok_and_writes_nothing(ctx):
    rows, cols = 20, 33
    orig, ed, scr = _images(rows, cols, 3)
    e, s = _Dev(ed), _Dev(scr)
    L = rt.lib()
    ep, epitch = C.c_void_p(e.img[0]), C.c_size_t(e.img[1]); sp, spitch = C.c_void_p(s.img[0]), C.c_size_t(s.img[1])
    assert L.rtdd_paint_strokes(ctx._h, None, C.c_int(0), ep, epitch, sp, spitch, None, C.c_size_t(0), C.c_int(rows), C.c_int(cols)) == 0
    one = (rt.Stroke * 1)(rt.Stroke(5, 5, 9, 9, 7, 1, 3))
    assert L.rtdd_paint_strokes(ctx._h, one, C.c_int(0), ep, epitch, sp, spitch, None, C.c_size_t(0), C.c_int(rows), C.c_int(cols)) == 0
    ctx.synchronize()
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)


def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    orig, ed, scr = _images(rows, cols, 4)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    L = rt.lib()
    good = rt.Stroke(5, 5, 9, 9, 7, 1, 3)

    def call(strokes=(good,), count=None, edited=e.img, scribble=s.img, original=o.img, r=rows, c=cols, null_strokes=False):
        arr = (rt.Stroke * max(len(strokes), 1))(*strokes)
        n = len(strokes) if count is None else count
        return L.rtdd_paint_strokes(ctx._h, None if null_strokes else arr, C.c_int(n), *raw_target(edited, scribble, original, r, c))

    def S(**kw):
        f = dict(x0=5, y0=5, x1=9, y1=9, radius=7, brush=1, label=3); f.update(kw)
        return rt.Stroke(f["x0"], f["y0"], f["x1"], f["y1"], f["radius"], f["brush"], f["label"])
    big = [good] * 4097
    refused = {
        "null strokes with count > 0": call(null_strokes=True, count=1),
        "count < 0": call(count=-1),
        "count > 4096": call(strokes=big),
        "null edited": call(edited=None),
        "null scribble": call(scribble=None),
        "negative rows": call(r=-1),
        "negative cols": call(c=-1),
        "edited pitch": call(edited=(e.img[0], cols * 3 - 1)),
        "scribble pitch": call(scribble=(s.img[0], cols - 1)),
        "rows above 32768": call(r=32769),
        "cols above 32768": call(c=32769, edited=(e.img[0], 1 << 20), scribble=(s.img[0], 1 << 20)),
        "radius -1": call(strokes=(S(radius=-1),)),
        "radius 1025": call(strokes=(S(radius=1025),)),
        "brush 2": call(strokes=(S(brush=2),)),
        "brush -1": call(strokes=(S(brush=-1),)),
        "label 256": call(strokes=(S(label=256),)),
        "label -2": call(strokes=(S(label=-2),)),
        "erase without original": call(strokes=(S(label=-1),), original=None),
        "erase with a short original pitch": call(strokes=(S(label=-1),), original=(o.img[0], cols * 3 - 1)),
        "x0 too small": call(strokes=(S(x0=-32769),)),
        "y0 too large": call(strokes=(S(y0=32768),)),
        "x1 too large": call(strokes=(S(x1=32768),)),
        "y1 too small": call(strokes=(S(y1=-32769),)),
        "a bad stroke behind good ones": call(strokes=(good, good, S(radius=2000))),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    assert call() == 0 and call(original=None) == 0                  # (the good stroke alone is accepted, with or without an original)
    assert call(strokes=(S(x0=-32768, y0=32767, radius=1024, label=255),)) == 0 and call(strokes=(S(radius=0, label=0),)) == 0
    ctx.synchronize()


def test_stamps_in_one_call_are_the_calls_of_paint_image(ctx):
    rows, cols = 135, 241
    rng = np.random.default_rng(12)
    stamps = [(int(rng.integers(-10, cols + 10)), int(rng.integers(-10, rows + 10)), int(rng.integers(0, 256)), int(rng.integers(0, 40))) for _ in range(500)]
    orig, ed, scr = _images(rows, cols, 5)
    e1, s1, e2, s2 = _Dev(ed), _Dev(scr), _Dev(ed), _Dev(scr)
    for x, y, label, radius in stamps:
        ctx.GPUPaintImage(x, y, label, radius, e1.img, s1.img, rows, cols)
    ctx.paint_strokes([(x, y, x, y, radius, sr.BRUSH_SQUARE, label) for x, y, label, radius in stamps], e2.img, s2.img, rows, cols)
    ctx.synchronize()
    assert np.array_equal(e1.host(), e2.host()) and np.array_equal(s1.host(), s2.host()) and (s1.host() == 255).sum() > 1000


# ---- the eraser reaches the estimate ---------------------------------------------------------------------------------------------------
_refs = {}


def _band(ann):
    """An eraser band through the labels: a thick square stroke across the image at the labels' median row, and a round one down the middle."""
    rows, cols = ann.shape
    ys = np.nonzero(ann != 32)[0]
    y = int(np.median(ys))
    return [(-5, y, cols + 5, y + 6, rows // 5, sr.BRUSH_SQUARE, sr.STROKE_ERASE), (cols // 2, -3, cols // 2 + 20, rows + 3, 31, sr.BRUSH_ROUND, sr.STROKE_ERASE)]


def _reference(oracle, lut, contract):
    """(cascade after annotate + estimate + erase + rebuild + estimate, the same without the erasure) for the reduced pair."""
    if contract not in _refs:
        bgr, ann = _pair()
        erased = Cascade(oracle, bgr, ann, lut, contract, threads=oracle.max_threads())
        kept = Cascade(oracle, bgr, ann, lut, contract, threads=oracle.max_threads())
        assert erased.P >= 3
        erased.estimate(ITERS); kept.estimate(ITERS)
        first = {"depth": [d.copy() for d in erased.depth], "u8": erased.depth_u8.copy()}
        before = int((erased.scribble[0] == 255).sum())
        sr.paint_strokes(_band(ann), erased.edited[0], erased.scribble[0], bgr)
        after = int((erased.scribble[0] == 255).sum())
        assert 0 < after < before - 200, (before, after)
        sr.rebuild(erased)
        erased.estimate(ITERS); kept.estimate(ITERS)
        _refs[contract] = (erased, kept, first)
    return _refs[contract]


def _erase_on_the_pyramid(c, ann, rows, cols):
    sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
    c.paint_strokes(_band(ann), (ep[0], ep[1]), (sp[0], sp[1]), rows, cols, original=(op[0], op[1]))


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("contract", [1, 0])
def test_the_eraser_reaches_the_estimate(oracle, lut, contract, lds, batched):
    bgr, ann = _pair()
    rows, cols = ann.shape
    erased, kept, _ = _reference(oracle, lut, contract)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.set_option(rt.OPT_FP_CONTRACT, contract); c.set_option(rt.OPT_ANNOTATION_LDS, lds)
        dimg, dann = up(bgr), up(ann)
        if batched:
            assert c.pyramid_create_batch(rows, cols, 3) == erased.P
            for b in range(3):
                c.pyramid_select(b); c.pyramid_set_image(dimg); c.pyramid_set_annotation(dann)
            c.estimate_depth_batch(ITERS)
            c.pyramid_select(1)
            _erase_on_the_pyramid(c, ann, rows, cols)
            c.estimate_depth_batch(ITERS); c.synchronize()
            _assert_pyramid(c, erased, "the erased image of the batch")
            for b in (0, 2):
                c.pyramid_select(b)
                _assert_pyramid(c, kept, f"image {b} of the batch, which lost nothing")
            return
        assert c.pyramid_create(rows, cols) == erased.P
        c.pyramid_set_image(dimg); c.pyramid_set_annotation(dann)
        c.estimate_depth(ITERS)
        _erase_on_the_pyramid(c, ann, rows, cols)
        c.estimate_depth(ITERS); c.synchronize()
        _assert_pyramid(c, erased, f"contract {contract}, lds {lds}")
        if contract == 1:
            # not vacuous: the same sequence WITHOUT the rebuild -- level 0 cleared by rtdd_upload, which accumulates -- keeps erased labels
            # on the coarse levels
            with rt.Context(0) as d:
                d.GPULoadWeights(0.4); d.set_option(rt.OPT_ANNOTATION_LDS, lds)
                d.pyramid_create(rows, cols); d.pyramid_set_image(dimg); d.pyramid_set_annotation(dann)
                d.estimate_depth(ITERS)
                for kind, host in ((rt.IMG_SCRIBBLE, erased.scribble[0]), (rt.IMG_EDITED, erased.edited[0])):
                    ptr, pitch, _, _ = d.pyramid_image(kind, 0)
                    w = host.size // rows
                    d._check(rt.lib().rtdd_upload(d._h, C.c_void_p(ptr), C.c_size_t(pitch), C.c_void_p(np.ascontiguousarray(host).ctypes.data), C.c_size_t(w), C.c_size_t(w), C.c_int(rows)))
                d.pyramid_annotation_changed()
                d.estimate_depth(ITERS); d.synchronize()
                assert np.array_equal(d.pyramid_download(rt.IMG_SCRIBBLE, 0), erased.scribble[0])
                stale = sum(int((d.pyramid_download(rt.IMG_SCRIBBLE, l) != erased.scribble[l]).sum()) for l in range(1, erased.P))
                assert stale >= 1, "without the rebuild the coarse levels should still hold the erased labels"
                # ... and the explicit call mends exactly that
                d.pyramid_annotation_rebuild()
                d.estimate_depth(ITERS); d.synchronize()
                for l in range(erased.P):
                    assert np.array_equal(d.pyramid_download(rt.IMG_SCRIBBLE, l), erased.scribble[l]), f"after the explicit rebuild: scribble {l}"
                    assert np.array_equal(d.pyramid_download(rt.IMG_EDITED, l), erased.edited[l]), f"after the explicit rebuild: edited {l}"


def _live_sequence(oracle, lut, bgr, ann, frames, reduced_from):
    """u8 maps of `frames` live frames: the full pair, and from frame `reduced_from` on the pair with the band erased (rebuild there)."""
    ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
    full = (ref.scribble[0].copy(), ref.edited[0].copy())
    s2, e2 = full[0].copy(), full[1].copy()
    sr.paint_strokes(_band(ann), e2, s2, bgr)
    maps = []
    for n in range(frames):
        s, e = full if n < reduced_from else (s2, e2)
        ref.scribble[0][...] = s; ref.edited[0][...] = e
        if n == reduced_from:
            sr.rebuild(ref)
        ref.estimate(ITERS)
        maps.append(ref.depth_u8.copy())
    return full, (s2, e2), maps, ref


@pytest.mark.parametrize("in_flight,force", [(1, 0), (2, 0), (2, 1)])
def test_live_frames_with_fewer_labels_after_a_rebuild(oracle, lut, in_flight, force):
    """Frame 3 uploads a pair with fewer labels and rtdd_pyramid_annotation_rebuild was called in front of it: every frame's map is the
    restated sequence's, one frame at a time and two in flight -- and (force) when the rebuilt frame's first blocked launch is made to report
    a time-out (RTDD_OPT_DEBUG_FORCE_STATUS: a stored status word, no fault), so that it and the frame behind it are run again."""
    bgr, ann = _pair()
    rows, cols = ann.shape
    frames = 5
    full, reduced, maps, ref = _live_sequence(oracle, lut, bgr, ann, frames, 3)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.synchronize()
        h = [rt.host_image((rows, cols)), rt.host_image((rows, cols, 3)), rt.host_image((rows, cols)), rt.host_image((rows, cols, 3))]
        out = [rt.host_image((rows, cols)) for _ in range(2)]
        h[0].a[...] = full[0]; h[1].a[...] = full[1]; h[2].a[...] = reduced[0]; h[3].a[...] = reduced[1]
        got = []
        for n in range(frames):
            while c.live_pending() >= in_flight:
                k = len(got); c.live_wait(); got.append(out[k % 2].a.copy())
            if n == 3:
                c.pyramid_annotation_rebuild()
                if force:
                    c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
            s, e = (h[0], h[1]) if n < 3 else (h[2], h[3])
            c.live_submit(s.a, e.a, out[n % 2].a, ITERS)
        while c.live_pending():
            k = len(got); c.live_wait(); got.append(out[k % 2].a.copy())
        c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == force
        for n in range(frames):
            print(f"frame {n}: {int((got[n] != maps[n]).sum())} pixels differ")
        for n in range(frames):
            assert np.array_equal(got[n], maps[n]), f"frame {n}"
        for l in range(ref.P):
            assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE, l), ref.scribble[l]), f"scribble {l} after the last frame"
        for x in h + out:
            x.free()


def test_an_erase_then_estimate_heals_to_the_same_bits(oracle, lut):
    """The erase-then-estimate sequence with RTDD_OPT_DEBUG_FORCE_STATUS = 1 (the one-shot testing aid: a status word stored behind the
    next blocked launch, no fault): the estimate that rebuilt is run again with the rebuild and gives the bits of an undisturbed run."""
    bgr, ann = _pair()
    rows, cols = ann.shape
    erased, _, first = _reference(oracle, lut, 1)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS); c.synchronize()
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, 0), first["depth"][0], "first estimate")
        _erase_on_the_pyramid(c, ann, rows, cols)
        c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
        c.estimate_depth(ITERS); c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        _assert_pyramid(c, erased, "healed erase-then-estimate")
