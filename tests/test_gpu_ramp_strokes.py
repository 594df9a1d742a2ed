"""rtdd_paint_ramp_strokes on the GPU, through the C ABI, the harness' --ramp / --ramp-at included (-m gpu): every comparison is byte
equality of both images against tests/ramp_ref.py (or, for whole estimates, of every level against the restated cascade fed with the
restated annotation).  The shapes are small: the label rule has no size-dependent path, and the tiles, the cull and the walk are
tests/test_gpu_strokes.py's (tests/paint_gpu.py has the helpers of both)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ramp_ref as rr
import realtimedepthdiffusion_amd as rt
import roi_util
import strokes_ref as sr
from cascade_ref import Cascade
from golden_util import NAMES, load
from gpu_util import up
from paint_gpu import ctx  # noqa: F401
from paint_gpu import ITERS, _assert_pyramid, _cascade, _Dev, _images, _pair, _polyline, raw_target, sub_views
from paint_gpu import _flag as _stroke_flag
from test_gpu_harness import BIN, ROOT, _read_pnm, _write_pnm

pytestmark = pytest.mark.gpu
HALF_TIES, extreme_strokes = rr.HALF_TIES, rr.extreme_strokes


def _ramps(rng, rows, cols, n):
    """test_gpu_strokes' random walk (both brushes, erasers, stamps, strokes partly and wholly outside, a few across the whole domain) with
    a second label: a third of the painting strokes rise, a third fall, a third are constant."""
    out = []
    for i, q in enumerate(_polyline(rng, rows, cols, n)):
        if q[6] == sr.STROKE_ERASE:
            out.append(q + (sr.STROKE_ERASE,))
        elif i % 3 == 0:
            out.append(q + (q[6],))
        else:
            a, b = sorted((q[6], int(rng.integers(0, 256))))
            out.append(q[:6] + ((a, b) if i % 3 == 1 else (b, a)))
    return out


def _run(c, strokes, e, s, o, rows, cols):
    c.paint_ramp_strokes(strokes, e.img, s.img, rows, cols, original=o.img if o is not None else None)
    c.synchronize()


def _check(c, strokes, rows, cols, seed, what=""):
    orig, ed, scr = _images(rows, cols, seed)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    _run(c, strokes, e, s, o, rows, cols)
    rr.paint_ramp_strokes(strokes, ed, scr, orig)
    got_e, got_s = e.host(), s.host()
    print(f"{what}{rows}x{cols}, {len(strokes)} strokes: scribble differs at {int((got_s != scr).sum())}, edited at {int((got_e != ed).any(-1).sum())} pixels; "
          f"{int((scr == 255).sum())} labelled, {len(np.unique(ed[scr == 255]))} labels")
    assert np.array_equal(got_s, scr) and np.array_equal(got_e, ed), what
    assert np.array_equal(o.host(), orig)
    return ed, scr


@pytest.mark.parametrize("rows,cols,n,seed", [(1, 1, 1, 1), (1, 1, 64, 2), (1, 300, 2, 3), (1, 300, 300, 4), (67, 45, 1, 5), (67, 45, 64, 6), (67, 45, 256, 7),
                                              (67, 45, 257, 8), (67, 45, 4096, 9), (33, 130, 64, 10)])
def test_ramp_polylines_match_the_restatement(ctx, rows, cols, n, seed):
    strokes = _ramps(np.random.default_rng(seed), rows, cols, n)
    assert len(strokes) == n
    _check(ctx, strokes, rows, cols, seed)


def test_extreme_geometry_and_half_ties(ctx):
    rows, cols = 67, 45
    many = 0
    for i, q in enumerate(extreme_strokes()):
        ed, scr = _check(ctx, [q], rows, cols, 40 + i, f"{q}: ")
        assert (scr == 255).all()
        many = max(many, len(np.unique(ed)))
    assert many > 40                                                  # (the shifted segments: the image sees many labels of one stroke)
    ed, scr = _check(ctx, HALF_TIES, rows, cols, 60, "half ties: ")
    assert list(ed[0, :3, 0]) == [0, 1, 1]
    for q in HALF_TIES:
        _check(ctx, [q], rows, cols, 61, f"{q}: ")


def test_equal_labels_are_the_existing_call_byte_for_byte(ctx):
    for rows, cols, n, seed in ((67, 45, 300, 70), (33, 130, 64, 71), (1, 300, 40, 72)):
        plain = _polyline(np.random.default_rng(seed), rows, cols, n)
        assert any(q[6] == sr.STROKE_ERASE for q in plain)
        orig, ed, scr = _images(rows, cols, seed)
        o, e1, s1, e2, s2 = _Dev(orig), _Dev(ed), _Dev(scr), _Dev(ed), _Dev(scr)
        ctx.paint_strokes(plain, e1.img, s1.img, rows, cols, original=o.img)
        _run(ctx, [q + (q[6],) for q in plain], e2, s2, o, rows, cols)
        assert np.array_equal(e1.host(), e2.host()) and np.array_equal(s1.host(), s2.host())
        assert (s1.host() == 255).any()


def test_reversed_ends_with_swapped_labels_on_the_device(ctx):
    rows, cols = 67, 45
    strokes = [q for q in _ramps(np.random.default_rng(80), rows, cols, 200)] + HALF_TIES + extreme_strokes()[8:]
    back = [(q[2], q[3], q[0], q[1], q[4], q[5], q[7], q[6]) for q in strokes]
    orig, ed, scr = _images(rows, cols, 80)
    o, e1, s1, e2, s2 = _Dev(orig), _Dev(ed), _Dev(scr), _Dev(ed), _Dev(scr)
    _run(ctx, strokes, e1, s1, o, rows, cols)
    _run(ctx, back, e2, s2, o, rows, cols)
    assert np.array_equal(e1.host(), e2.host()) and np.array_equal(s1.host(), s2.host())
    rr.paint_ramp_strokes(strokes, ed, scr, orig)
    assert np.array_equal(e1.host(), ed)


@pytest.mark.parametrize("layout", roi_util.LAYOUTS_U8, ids=lambda l: f"lead{l[0]}_pitch+{l[1]}")
def test_sub_image_views(ctx, layout):
    """The three images inside larger allocations, odd lead bytes and pitches: nothing outside the views is written, nothing uncovered
    inside them, and the original not at all."""
    rows, cols = 37, 75
    lead, residue = layout
    orig, ed, scr = _images(rows, cols, 90 + lead)
    scr[::3, ::5] = 255
    strokes = _ramps(np.random.default_rng(90 + lead + residue), rows, cols, 24)        # (fewer than 64: none of the walk's image-wide strokes)
    o, e, s = sub_views(orig, ed, scr, layout)
    ctx.paint_ramp_strokes(strokes, e.img, s.img, rows, cols, original=o.img)
    ctx.synchronize()
    rr.paint_ramp_strokes(strokes, ed, scr, orig)
    assert np.array_equal(e.result(), ed) and np.array_equal(s.result(), scr)
    o.assert_unchanged()
    touched = (ed != _images(rows, cols, 90 + lead)[1]).any(-1)
    assert 0 < touched.sum() < rows * cols                            # (some pixels no stroke covers: they must keep their bytes)


def test_every_refusal_is_invalid_and_leaves_the_images_alone(ctx):
    rows, cols = 20, 33
    orig, ed, scr = _images(rows, cols, 4)
    o, e, s = _Dev(orig), _Dev(ed), _Dev(scr)
    L = rt.lib()
    good = rt.RampStroke(5, 5, 9, 9, 7, 1, 3, 200)

    def call(strokes=(good,), count=None, edited=e.img, scribble=s.img, original=o.img, r=rows, c=cols, null_strokes=False):
        arr = (rt.RampStroke * max(len(strokes), 1))(*strokes)
        n = len(strokes) if count is None else count
        return L.rtdd_paint_ramp_strokes(ctx._h, None if null_strokes else arr, C.c_int(n), *raw_target(edited, scribble, original, r, c))

    def S(**kw):
        f = dict(x0=5, y0=5, x1=9, y1=9, radius=7, brush=1, label0=3, label1=200); f.update(kw)
        return rt.RampStroke(*(f[k] for k in ("x0", "y0", "x1", "y1", "radius", "brush", "label0", "label1")))
    refused = {
        "null strokes with count > 0": call(null_strokes=True, count=1),
        "count < 0": call(count=-1),
        "count > 4096": call(strokes=[good] * 4097),
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
        "label0 256": call(strokes=(S(label0=256),)),
        "label1 256": call(strokes=(S(label1=256),)),
        "label0 -2": call(strokes=(S(label0=-2),)),
        "label1 -2": call(strokes=(S(label1=-2),)),
        "only label0 erases": call(strokes=(S(label0=-1),)),
        "only label1 erases": call(strokes=(S(label1=-1),)),
        "erase without original": call(strokes=(S(label0=-1, label1=-1),), original=None),
        "erase with a short original pitch": call(strokes=(S(label0=-1, label1=-1),), original=(o.img[0], cols * 3 - 1)),
        "x0 too small": call(strokes=(S(x0=-32769),)),
        "y0 too large": call(strokes=(S(y0=32768),)),
        "x1 too large": call(strokes=(S(x1=32768),)),
        "y1 too small": call(strokes=(S(y1=-32769),)),
        "a bad stroke behind good ones": call(strokes=(good, good, S(label1=-1))),
    }
    ctx.synchronize()
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    # count == 0 is OK and writes nothing, with or without an array
    assert call(count=0) == 0 and call(null_strokes=True, count=0) == 0
    ctx.synchronize()
    assert np.array_equal(e.host(), ed) and np.array_equal(s.host(), scr)
    assert call() == 0 and call(original=None) == 0 and call(strokes=(S(label0=-1, label1=-1),)) == 0
    assert call(strokes=(S(x0=-32768, y0=32767, radius=1024, label0=255, label1=0),)) == 0 and call(strokes=(S(radius=0, label0=0, label1=0),)) == 0
    ctx.synchronize()


# ---- the ramp reaches the estimate -----------------------------------------------------------------------------------------------------
_refs = {}


def _annotation(ann):
    """A ramp down the image through the labels, an eraser band across it, a second ramp over the band: the last stroke decides."""
    rows, cols = ann.shape
    y = int(np.median(np.nonzero(ann != 32)[0]))
    return [(cols // 3, 10, cols // 3 + 40, rows - 10, 9, sr.BRUSH_ROUND, 20, 240), (-5, y, cols + 5, y + 6, rows // 6, sr.BRUSH_SQUARE, sr.STROKE_ERASE, sr.STROKE_ERASE),
            (cols - 20, y - 30, 30, y + 30, 5, sr.BRUSH_SQUARE, 200, 64)]


def _reference(oracle, lut, contract):
    if contract not in _refs:
        bgr, ann = _pair()
        ref = Cascade(oracle, bgr, ann, lut, contract, threads=oracle.max_threads())
        assert ref.P >= 3
        ref.estimate(ITERS)
        before = ref.scribble[0].copy()
        rr.paint_ramp_strokes(_annotation(ann), ref.edited[0], ref.scribble[0], bgr)
        assert ((before == 255) & (ref.scribble[0] == 0)).sum() > 200 and ((before != 255) & (ref.scribble[0] == 255)).sum() > 200
        assert len(np.unique(ref.edited[0][ref.scribble[0] == 255])) > 100
        sr.rebuild(ref)                                               # a record of the call erases: the call asks for the rebuild itself
        ref.estimate(ITERS)
        _refs[contract] = ref
    return _refs[contract]


@pytest.mark.parametrize("contract", [1, 0])
def test_a_ramp_call_then_an_estimate(oracle, lut, contract):
    bgr, ann = _pair()
    rows, cols = ann.shape
    ref = _reference(oracle, lut, contract)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.set_option(rt.OPT_FP_CONTRACT, contract)
        assert c.pyramid_create(rows, cols) == ref.P
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS)
        sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
        c.paint_ramp_strokes(_annotation(ann), (ep[0], ep[1]), (sp[0], sp[1]), rows, cols, original=(op[0], op[1]))
        c.estimate_depth(ITERS); c.synchronize()
        _assert_pyramid(c, ref, f"contract {contract}")


def test_live_frames_with_a_ramp_painted_on_the_host_pair(oracle, lut, ctx):
    """Four live frames, one in flight; in front of frame 2 the host paints a ramp on its own pair (here: with the library, on a device copy
    of it).  Every frame is the restated sequence's."""
    bgr, ann = _pair()
    rows, cols = ann.shape
    ramp = [(20, 20, cols - 30, rows - 25, 13, sr.BRUSH_ROUND, 250, 10), (cols - 10, 5, cols - 60, rows // 2, 8, sr.BRUSH_SQUARE, 0, 90)]
    ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
    first = (ref.scribble[0].copy(), ref.edited[0].copy())
    e, s = _Dev(first[1]), _Dev(first[0])
    _run(ctx, ramp, e, s, None, rows, cols)
    painted = (s.host(), e.host())
    want_e, want_s = first[1].copy(), first[0].copy()
    rr.paint_ramp_strokes(ramp, want_e, want_s)
    assert np.array_equal(painted[0], want_s) and np.array_equal(painted[1], want_e) and (want_s != first[0]).sum() > 1000
    maps = []
    for n in range(4):
        pair = first if n < 2 else painted
        ref.scribble[0][...] = pair[0]; ref.edited[0][...] = pair[1]
        ref.estimate(ITERS)
        maps.append(ref.depth_u8.copy())
    assert not np.array_equal(maps[1], maps[2])
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.synchronize()
        hs, he, out = rt.host_image((rows, cols)), rt.host_image((rows, cols, 3)), rt.host_image((rows, cols))
        got = []
        for n in range(4):
            pair = first if n < 2 else painted
            hs.a[...] = pair[0]; he.a[...] = pair[1]
            c.live_submit(hs.a, he.a, out.a, ITERS)
            c.live_wait()
            got.append(out.a.copy())
        c.synchronize()
        for n in range(4):
            print(f"frame {n}: {int((got[n] != maps[n]).sum())} pixels differ")
        for n in range(4):
            assert np.array_equal(got[n], maps[n]), f"frame {n}"
        for x in (hs, he, out):
            x.free()


# ---- the harness -------------------------------------------------------------------------------------------------------------------------
def _flag(q, frame=None):
    if q[6] == q[7]:
        return _stroke_flag(q[:7], frame)
    x0, y0, x1, y1, radius, brush, l0, l1 = q
    return ["--ramp" + ("" if frame is None else "-at"), ("" if frame is None else f"{frame}:") + f"{x0},{y0},{x1},{y1},{l0},{l1},{radius}" + (",round" if brush == sr.BRUSH_ROUND else "")]


def test_harness_ramp_is_the_python_api(tmp_path):
    """--stroke, --ramp, --erase, --ramp in command-line order, one rtdd_paint_ramp_strokes call: the annotated image and the map are what the
    same records through the Python API give (and the annotated image the restatement's)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[0])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    rows, cols = g["annotation"].shape
    strokes = [(10, 200, 240, 180, 11, sr.BRUSH_ROUND, 254, 254), (30, 20, 220, 240, 17, sr.BRUSH_ROUND, 10, 250), (-20, 128, 300, 120, 40, sr.BRUSH_SQUARE, -1, -1),
               (250, 100, 5, 140, 9, sr.BRUSH_SQUARE, 255, 0)]
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", "200"]
    for q in strokes:
        args += _flag(q)
    assert args.count("--ramp") == 2
    subprocess.check_output(args, text=True)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(g["bgr"])); c.pyramid_set_annotation(up(g["annotation"]))
        sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
        before_e, before_s = c.pyramid_download(rt.IMG_EDITED, 0), c.pyramid_download(rt.IMG_SCRIBBLE, 0)
        c.paint_ramp_strokes(strokes, (ep[0], ep[1]), (sp[0], sp[1]), rows, cols, original=(op[0], op[1]))
        c.estimate_depth(200); c.synchronize()
        edited, depth = c.pyramid_download(rt.IMG_EDITED, 0), c.pyramid_download(rt.IMG_DEPTH_U8)
    rr.paint_ramp_strokes(strokes, before_e, before_s, g["bgr"])
    assert np.array_equal(edited, before_e) and len(np.unique(before_e[before_s == 255])) > 100
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), edited[..., ::-1])
    assert np.array_equal(_read_pnm(tmp_path / "DepthMap.pgm"), depth)


def test_harness_ramp_in_a_live_view(tmp_path):
    """--live 4 --ramp-at 2:...: the harness paints its own host pair by the restated label rule; it runs, reports frames/s, and every frame
    is the restated cascade's."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[1])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    at = {2: [(30, 40, 200, 220, 9, sr.BRUSH_ROUND, 240, 15), (250, 10, 180, 100, 6, sr.BRUSH_SQUARE, 3, 180)]}
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--live", "4", "--iters", "200", "--write-all"]
    for f, qs in at.items():
        for q in qs:
            args += _flag(q, f)
    out = subprocess.check_output(args, text=True)
    assert "Live:" in out and "frames/s" in out, out
    _, c = _cascade(g)
    for n in range(4):
        rr.paint_ramp_strokes(at.get(n, ()), c.edited[0], c.scribble[0], g["bgr"])
        c.estimate(200)
        assert np.array_equal(_read_pnm(tmp_path / f"DepthMap_{n}.pgm"), c.depth_u8), f"frame {n}"
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
