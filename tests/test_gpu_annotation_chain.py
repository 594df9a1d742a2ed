"""Every instantiation of the one-launch annotation pyramid (image_kernels.hip), accumulating and rebuilding, on the GPU (-m gpu): the
chain in LDS at each depth it is compiled for (TOP = 1 .. 5) and the chain through global memory (RTDD_OPT_ANNOTATION_LDS = 0) on the
same shapes.  The shapes are the smallest with each pyramid depth, odd, so that every level size is a true floor and the last footprints
are ragged.  Per case: a sparse annotation, an estimate, strokes on the pyramid's own level-0 pair (accumulate), an estimate, an eraser
band (the implicit rebuild), an estimate, an uploaded pair with fewer labels behind rtdd_pyramid_annotation_rebuild, an estimate -- and
after each estimate every level's scribble and edited image byte for byte against the restatement (oracle.pyrdown_annotation,
strokes_ref).  The two smallest shapes also compare every depth level bit for bit with the whole restated cascade: the coarsest level's
injection is part of the kernel."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import strokes_ref as sr
from cascade_ref import Cascade, pyramid_levels
from gpu_util import assert_bit_equal, up

pytestmark = pytest.mark.gpu
ITERS = 64
SHAPES = [(91, 133, 1), (181, 203, 2), (363, 377, 3), (725, 731, 4), (1443, 1451, 5)]           # rows, cols, TOP = levels - 1
CASES = [s + (1,) for s in SHAPES] + [SHAPES[0] + (2,)]                                          # ... and images in the batch
_refs = {}


def _pair(rows, cols, seed):
    """A random image and a sparse annotation (32 = no label) with labels in the last row and the last column, the corner included."""
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    lab = rng.random((rows, cols)) < 0.003
    lab[rows - 1, ::7] = True; lab[::5, cols - 1] = True; lab[rows - 1, cols - 1] = True
    values = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    values[values == 32] = 33
    return bgr, np.where(lab, values, 32).astype(np.uint8)


def _strokes(rows, cols, image):
    return [(cols // 7, rows // 6, cols - cols // 5, rows - rows // 4, 5, sr.BRUSH_ROUND, 40 + image),
            (3, rows - 1 - rows // 9, cols + 10, rows - 1 - rows // 9, 4, sr.BRUSH_SQUARE, 200),
            (cols - 2, rows - 2, cols - 2, rows - 2, 7, sr.BRUSH_SQUARE, 90 + image)]


def _band(rows, cols):
    """An eraser band across the image, thick enough to empty whole footprints of the coarsest level, and a round one down the middle."""
    return [(-5, rows // 2, cols + 5, rows // 2 + 6, rows // 5, sr.BRUSH_SQUARE, sr.STROKE_ERASE), (cols // 2, -3, cols // 2 + 20, rows + 3, 31, sr.BRUSH_ROUND, sr.STROKE_ERASE)]


def _down(oracle, scribble, edited):
    for l in range(1, len(scribble)):
        oracle.pyrdown_annotation(scribble[l - 1], edited[l - 1], scribble[l], edited[l])


def _reference(oracle, lut, rows, cols, image):
    """The restated sequence for image `image` of a batch of this shape: bgr, annotation, the pair uploaded in front of the last estimate,
    and after each of the four estimates (scribble levels, edited levels, depth levels or None)."""
    key = (rows, cols, image)
    if key in _refs:
        return _refs[key]
    bgr, ann = _pair(rows, cols, 1000 * image + rows)
    whole = rows * cols < 40000                                       # the two smallest shapes: the solves too
    ref = Cascade(oracle, bgr, ann, lut, 1, threads=oracle.max_threads())
    assert ref.P == pyramid_levels(rows, cols)
    assert (ref.scribble[0][rows - 1] == 255).any() and (ref.scribble[0][:, cols - 1] == 255).any() and ref.scribble[0][rows - 1, cols - 1] == 255
    steps = []

    def estimate():
        if whole:
            ref.estimate(ITERS)
        else:
            _down(oracle, ref.scribble, ref.edited)
        steps.append(([s.copy() for s in ref.scribble], [e.copy() for e in ref.edited], [d.copy() for d in ref.depth] if whole else None))

    estimate()
    assert all((ref.scribble[l] == 255).any() for l in range(1, ref.P)), "a coarse level without a label"
    sr.paint_strokes(_strokes(rows, cols, image), ref.edited[0], ref.scribble[0], bgr)
    estimate()
    sr.paint_strokes(_band(rows, cols), ref.edited[0], ref.scribble[0], bgr)
    acc_s, acc_e = [s.copy() for s in ref.scribble], [e.copy() for e in ref.edited]       # what accumulating in place of the rebuild would give
    _down(oracle, acc_s, acc_e)
    sr.rebuild(ref)
    estimate()
    for l in range(1, ref.P):
        assert not np.array_equal(acc_s[l], ref.scribble[l]), f"level {l}: accumulating and rebuilding give the same scribble"
    s7, e7 = ref.scribble[0].copy(), ref.edited[0].copy()
    yy, xx = np.indices((rows, cols))
    drop = (s7 == 255) & ((xx + yy) % 2 == 0)
    assert 0 < drop.sum() < (s7 == 255).sum()
    s7[drop] = 0; e7[drop] = bgr[drop]
    ref.scribble[0][...] = s7; ref.edited[0][...] = e7
    sr.rebuild(ref)
    estimate()
    _refs[key] = (bgr, ann, (s7, e7), steps)
    return _refs[key]


def _upload(c, host, ptr, pitch):
    host = np.ascontiguousarray(host)
    rows, width = host.shape[0], host.size // host.shape[0]
    c._check(rt.lib().rtdd_upload(c._h, C.c_void_p(ptr), C.c_size_t(pitch), C.c_void_p(host.ctypes.data), C.c_size_t(width), C.c_size_t(width), C.c_int(rows)))


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("rows,cols,top,images", CASES)
def test_accumulate_and_rebuild_at_every_depth(oracle, lut, rows, cols, top, images, lds):
    assert pyramid_levels(rows, cols) == top + 1
    refs = [_reference(oracle, lut, rows, cols, b) for b in range(images)]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.set_option(rt.OPT_ANNOTATION_LDS, lds)
        assert (c.pyramid_create_batch(rows, cols, images) if images > 1 else c.pyramid_create(rows, cols)) == top + 1

        def each():
            for b in range(images):
                if images > 1:
                    c.pyramid_select(b)
                yield b, refs[b]

        def level0():
            sp = c.pyramid_image(rt.IMG_SCRIBBLE, 0); ep = c.pyramid_image(rt.IMG_EDITED, 0); op = c.pyramid_image(rt.IMG_ORIGINAL, 0)
            return (ep[0], ep[1]), (sp[0], sp[1]), (op[0], op[1])

        def estimate_and_check(step, what):
            c.estimate_depth_batch(ITERS) if images > 1 else c.estimate_depth(ITERS)
            c.synchronize()
            for b, ref in each():
                scribble, edited, depth = ref[3][step]
                for l in range(top + 1):
                    assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE, l), scribble[l]), f"{what}, image {b}: scribble {l}"
                    assert np.array_equal(c.pyramid_download(rt.IMG_EDITED, l), edited[l]), f"{what}, image {b}: edited {l}"
                    if depth is not None:
                        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), depth[l], f"{what}, image {b}: depth {l}")

        for b, ref in each():
            c.pyramid_set_image(up(ref[0])); c.pyramid_set_annotation(up(ref[1]))
        estimate_and_check(0, "the annotation as set")
        for b, ref in each():
            e, s, _ = level0()
            c.paint_strokes(_strokes(rows, cols, b), e, s, rows, cols)
        estimate_and_check(1, "strokes accumulated")
        for b, ref in each():
            e, s, o = level0()
            c.paint_strokes(_band(rows, cols), e, s, rows, cols, original=o)
        estimate_and_check(2, "a band erased")
        for b, ref in each():
            e, s, _ = level0()
            _upload(c, ref[2][0], *s); _upload(c, ref[2][1], *e)
        c.pyramid_annotation_rebuild()
        estimate_and_check(3, "fewer labels uploaded and the rebuild asked for")
