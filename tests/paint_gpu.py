"""Scaffolding shared by the paint calls' -m gpu tests (tests/test_gpu_{strokes,ramp_strokes,fill_polygon,harness_strokes,harness_fill}.py):
pitched device images with padded rows, random images and the random walk of strokes, the context as a fixture, the three images as
sub-image views, the image arguments of the raw ABI, the reduced Dog pair and the comparison of a whole pyramid with the restated
cascade, and the harness' stroke flags.  What is particular to a call -- its records, its restatement, its refusals -- stays in its own
file."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import roi_util
import strokes_ref as sr
from dataset_util import load_pair
from gpu_util import assert_bit_equal

PAD = 0xA5
ITERS = 300


class _Dev:
    """A pitched device image with padded rows (every padding byte PAD)."""

    def __init__(self, host):
        import torch
        host = np.ascontiguousarray(host)
        self.rows = host.shape[0]
        self.width = int(np.prod(host.shape[1:]))
        self.pitch = (self.width + 255) // 256 * 256 + 256
        self.base = torch.full((self.rows, self.pitch), PAD, dtype=torch.uint8, device="cuda:0")
        self.base[:, :self.width] = torch.from_numpy(host.reshape(self.rows, self.width)).to("cuda:0")
        self.shape = host.shape

    @property
    def img(self):
        return (self.base.data_ptr(), self.pitch)

    def host(self):
        a = self.base.cpu().numpy()
        assert (a[:, self.width:] == PAD).all(), "row padding was written"
        return np.ascontiguousarray(a[:, :self.width]).reshape(self.shape)


def _images(rows, cols, seed):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    return orig, orig.copy(), np.zeros((rows, cols), np.uint8)


def _polyline(rng, rows, cols, n, long_ones=True):
    """n segments of a random walk that starts inside and may leave the image: brushes, radii, labels and erasures mixed; it crosses itself,
    so the order of the strokes matters.  A few strokes reach far outside."""
    out = []
    x, y = int(rng.integers(0, cols)), int(rng.integers(0, rows))
    step = max(4, min(60, max(rows, cols) // 8))
    for i in range(n):
        nx = int(np.clip(x + rng.integers(-step, step + 1), -40, cols + 40))
        ny = int(np.clip(y + rng.integers(-step, step + 1), -40, rows + 40))
        if i % 7 == 3:
            nx, ny = x, y                                            # a stamp in the middle of the drag
        label = sr.STROKE_ERASE if rng.random() < 0.25 else int(rng.integers(0, 256))
        out.append((x, y, nx, ny, int(rng.integers(0, 32)), int(rng.integers(0, 2)), label))
        x, y = nx, ny
    if long_ones and n >= 64:
        out[n // 3] = (-32768, rows // 3, 32767, rows // 3 + 150, 9, sr.BRUSH_ROUND, 17)        # from far outside to far outside
        out[n // 2] = (cols // 2, -32768, cols // 2 - 90, 32767, 1024 if rows * cols < 3000000 else 40, sr.BRUSH_SQUARE, sr.STROKE_ERASE)
        if rows * cols <= 2100000:
            out[2 * n // 3] = (-32768, -32768, 32767, 32767, 300, sr.BRUSH_ROUND, 201)          # the diagonal of the domain
        out[n - 5] = (-500, -700, -300, -650, 64, sr.BRUSH_ROUND, 3)                            # wholly outside
    return out


@pytest.fixture(scope="module")
def ctx():
    with rt.Context(0) as c:
        yield c


def sub_views(orig, ed, scr, layout):
    """The three images inside larger allocations, odd lead bytes and pitches (a roi_util.LAYOUTS_U8 entry): (original, edited, scribble)
    as roi_util.Roi, the original an input, the pair outputs."""
    cols = scr.shape[1]
    lead, residue = layout
    o = roi_util.Roi(orig, lead, roi_util.pitch_for(cols * 3, lead, residue), roi_util.FILL_INPUT, what="original")
    e = roi_util.Roi(ed, (lead + 1) % 5, roi_util.pitch_for(cols * 3, (lead + 1) % 5, residue), roi_util.FILL_OUTPUT, seed=1, what="edited")
    s = roi_util.Roi(scr, lead, roi_util.pitch_for(cols, lead, (residue + 1) % 5), roi_util.FILL_OUTPUT, seed=2, what="scribble")
    return o, e, s


def raw_target(edited, scribble, original, rows, cols):
    """The last eight arguments of the paint calls of the raw ABI; an image is (pointer, pitch) or None."""
    ed_, sc_, or_ = (edited or (None, 0)), (scribble or (None, 0)), (original or (None, 0))
    return (C.c_void_p(ed_[0]), C.c_size_t(ed_[1]), C.c_void_p(sc_[0]), C.c_size_t(sc_[1]), C.c_void_p(or_[0]), C.c_size_t(or_[1]), C.c_int(rows), C.c_int(cols))


# ---- on a pyramid ----------------------------------------------------------------------------------------------------------------------------
def _pair():
    bgr, ann, _ = load_pair("Dog")
    return np.ascontiguousarray(bgr[::2, ::2]), np.ascontiguousarray(ann[::2, ::2])      # 336 x 312: three pyramid levels


def _assert_pyramid(c, ref, what):
    for l in range(ref.P):
        assert np.array_equal(c.pyramid_download(rt.IMG_SCRIBBLE, l), ref.scribble[l]), f"{what}: scribble {l}"
        assert np.array_equal(c.pyramid_download(rt.IMG_EDITED, l), ref.edited[l]), f"{what}: edited {l}"
    for l in range(ref.P - 1, -1, -1):
        assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), ref.depth[l], f"{what}: depth {l}")
    assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), ref.depth_u8), f"{what}: u8 map"


# ---- the harness ---------------------------------------------------------------------------------------------------------------------------
def _flag(q, frame=None):
    x0, y0, x1, y1, radius, brush, label = q
    head = "" if frame is None else f"{frame}:"
    tail = ",round" if brush == sr.BRUSH_ROUND else ""
    if label == sr.STROKE_ERASE:
        return ["--erase" + ("" if frame is None else "-at"), f"{head}{x0},{y0},{x1},{y1},{radius}{tail}"]
    return ["--stroke" + ("" if frame is None else "-at"), f"{head}{x0},{y0},{x1},{y1},{label},{radius}{tail}"]


def _cascade(g):
    import oracle
    from cascade_ref import Cascade
    return oracle, Cascade(oracle, g["bgr"], g["annotation"], oracle.load_weights(0.4), 1, threads=4)
