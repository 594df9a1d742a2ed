"""Depth-ramp strokes without a GPU: the restatement the GPU tests compare against (tests/ramp_ref.py) is pinned here -- the numpy label
rule against Python integers (the domain's corners and exact half ties included), its symmetry, its agreement with
strokes_ref.paint_strokes for equal labels -- the case that motivates the feature is solved with the numpy restatement of the solver,
the header and the Python mirror are checked to declare the new entry points, and rtdd_ramp_polyline (host arithmetic: no device) is
compared with its restatement through librtdd.so."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_restatement as npr
import ramp_ref as rr
import realtimedepthdiffusion_amd as rt
import strokes_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paint(rows, cols, strokes, seed=0, fn=rr.paint_ramp_strokes):
    orig = np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    e, s = orig.copy(), np.zeros((rows, cols), np.uint8)
    fn(strokes, e, s, orig)
    return e, s, orig


def _by_python_integers(rows, cols, strokes, seed=0):
    """The yardstick: strokes_ref.covers and ramp_ref.label_at, one pixel at a time, over the grown box of every stroke."""
    orig = np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    e, s = orig.copy(), np.zeros((rows, cols), np.uint8)
    for q in strokes:
        h = q[4] // 2
        for y in range(max(min(q[1], q[3]) - h, 0), min(max(q[1], q[3]) + h, rows - 1) + 1):
            for x in range(max(min(q[0], q[2]) - h, 0), min(max(q[0], q[2]) + h, cols - 1) + 1):
                if sr.covers(x, y, q):
                    if q[6] == rr.STROKE_ERASE:
                        e[y, x] = orig[y, x]; s[y, x] = 0
                    else:
                        e[y, x] = rr.label_at(x, y, q); s[y, x] = 255
    return e, s


HALF_TIES, extreme_strokes = rr.HALF_TIES, rr.extreme_strokes


def test_the_numpy_label_rule_is_the_integer_rule():
    rows, cols = 67, 45
    rng = np.random.default_rng(11)
    strokes = []
    for i in range(120):
        x0, y0 = int(rng.integers(-20, cols + 20)), int(rng.integers(-20, rows + 20))
        x1, y1 = (x0, y0) if i % 6 == 0 else (int(rng.integers(-20, cols + 20)), int(rng.integers(-20, rows + 20)))
        l0, l1 = (-1, -1) if i % 9 == 4 else (int(rng.integers(0, 256)), int(rng.integers(0, 256)))
        strokes.append((x0, y0, x1, y1, int(rng.integers(0, 30)), int(rng.integers(0, 2)), l0, l1))
    for group in (strokes, HALF_TIES):
        got = _paint(rows, cols, group, 1)
        want = _by_python_integers(rows, cols, group, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for q in extreme_strokes():                                       # one at a time: each covers the whole image
        got = _paint(rows, cols, [q], 2)
        want = _by_python_integers(rows, cols, [q], 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), q
        assert (got[1] == 255).all(), q
    seen = [len(np.unique(_paint(rows, cols, [q], 2)[0])) for q in extreme_strokes()]
    assert max(seen) > 40 and min(seen) == 1, seen                    # (whole-domain diagonals give the image one label, the shifted ones many)


def test_exact_half_ties_round_up():
    assert rr.label_at(1, 0, (0, 0, 2, 0, 1, 0, 0, 1)) == 1           # 0.5 -> 1
    assert rr.label_at(1, 0, (2, 0, 0, 0, 1, 0, 1, 0)) == 1           # the same stroke from its other end
    e, s, _ = _paint(3, 5, [(0, 0, 2, 0, 1, sr.BRUSH_SQUARE, 0, 1)])
    assert list(e[0, :3, 0]) == [0, 1, 1] and list(s[0]) == [255, 255, 255, 0, 0]
    ties = 0
    for q in HALF_TIES:                                               # horizontal, even length, odd label difference: a tie at the middle
        x0, y, x1, l0, l1 = q[0], q[1], q[2], q[6], q[7]
        assert (x1 - x0) % 2 == 0 and (l1 - l0) % 2 == 1
        mid = (x0 + x1) // 2
        assert 2 * rr.label_at(mid, y, q) == l0 + l1 + 1
        ties += 1
        for x in range(min(x0, x1) - 3, max(x0, x1) + 4):             # and beyond the ends: that end's label
            L = rr.label_at(x, y, q)
            assert min(l0, l1) <= L <= max(l0, l1)
            if (x - x0) * (x1 - x0) <= 0:
                assert L == l0
            if (x - x1) * (x0 - x1) <= 0:
                assert L == l1
    assert ties == 4


def _reverse(q):
    return (q[2], q[3], q[0], q[1], q[4], q[5], q[7], q[6])


def test_reversed_ends_with_swapped_labels_paint_the_same_images():
    rows, cols = 67, 45
    rng = np.random.default_rng(5)
    strokes = [(int(rng.integers(-30, 80)), int(rng.integers(-30, 90)), int(rng.integers(-30, 80)), int(rng.integers(-30, 90)), int(rng.integers(0, 40)),
                int(rng.integers(0, 2)), int(rng.integers(0, 256)), int(rng.integers(0, 256))) for _ in range(80)] + HALF_TIES + extreme_strokes()
    for q in strokes:
        for x, y in ((0, 0), (44, 66), (20, 30), (1, 0)):
            assert rr.label_at(x, y, q) == rr.label_at(x, y, _reverse(q)), q
    a = _paint(rows, cols, strokes[:84], 3)
    b = _paint(rows, cols, [_reverse(q) for q in strokes[:84]], 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for q in extreme_strokes():
        a, b = _paint(rows, cols, [q], 3), _paint(rows, cols, [_reverse(q)], 3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), q


def test_equal_labels_are_paint_strokes():
    rows, cols = 67, 45
    rng = np.random.default_rng(8)
    plain = []
    for i in range(150):
        x0, y0 = int(rng.integers(-20, cols + 20)), int(rng.integers(-20, rows + 20))
        x1, y1 = (x0, y0) if i % 7 == 0 else (x0 + int(rng.integers(-25, 26)), y0 + int(rng.integers(-25, 26)))
        plain.append((x0, y0, x1, y1, int(rng.integers(0, 24)), int(rng.integers(0, 2)), sr.STROKE_ERASE if rng.random() < 0.25 else int(rng.integers(0, 256))))
    assert any(q[6] == sr.STROKE_ERASE for q in plain)
    want = _paint(rows, cols, plain, 4, fn=sr.paint_strokes)
    got = _paint(rows, cols, [q + (q[6],) for q in plain], 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert 0 < (want[1] == 255).sum() < rows * cols


def test_one_ramp_beats_two_stamps_on_a_tiled_floor(lut):
    """The case that motivates the feature: a 48 x 40 image of 4-row bands (a tiled floor), the true surface the plane from label 40 at
    row 2 to label 200 at row 45.  Two constant stamps leave the diffusion to put the depth change at the bands' edges (a staircase); one
    ramp stroke carries the plane.  Measured with this restatement: mean |depth - plane| over rows 2..45 after 1000 sweeps 28.5 (stamps)
    against 5.45 (ramp); asserted: the ramp's is below half the stamps' -- a comparison, not a tuned threshold."""
    rows, cols = 48, 40
    levels = [60, 70, 140, 150, 156, 90, 95, 200, 205, 120, 126, 40]
    gray = np.repeat(np.array(levels, np.uint8), 4)[:, None].repeat(cols, 1)
    y0, y1, l0, l1 = 2, 45, 40, 200
    plane = l0 + (np.arange(rows) - y0) * (l1 - l0) / (y1 - y0)

    def deviation(strokes):
        e, s = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
        rr.paint_ramp_strokes(strokes, e, s)
        depth = np.where(s == 255, e[..., 0], 128).astype(np.float32)
        x = npr.solve(depth, s, gray, 1000, 0, 0, lut, 1)
        return float(np.abs(x[y0:y1 + 1] - plane[y0:y1 + 1, None]).mean()), s

    stamps, s_a = deviation([(5, y0, 7, y0, 3, sr.BRUSH_SQUARE, l0, l0), (5, y1, 7, y1, 3, sr.BRUSH_SQUARE, l1, l1)])   # two 3 x 5 stamps, columns 4..8
    ramp, s_b = deviation([(6, y0, 6, y1, 3, sr.BRUSH_SQUARE, l0, l1)])                                                 # 3 wide, columns 5..7
    assert (s_a == 255).sum() == 30 and np.array_equal(np.nonzero((s_a == 255).any(0))[0], np.arange(4, 9))
    assert (s_b == 255).sum() == 3 * 46 and np.array_equal(np.nonzero((s_b == 255).any(0))[0], np.arange(5, 8))
    print(f"mean |depth - plane| over rows {y0}..{y1} after 1000 sweeps: two stamps {stamps:.2f}, one ramp stroke {ramp:.2f}")
    assert ramp < 0.5 * stamps


def test_header_declares_the_struct_and_both_functions():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert "#define RTDD_VERSION 230" in header                     # found by symbol: no version bump
    body = re.search(r"typedef struct rtdd_ramp_stroke \{(.*?)\} rtdd_ramp_stroke;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.replace("int", "", 1).split(",")]
    assert fields == ["x0", "y0", "x1", "y1", "radius", "brush", "label0", "label1"]
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int rtdd_paint_ramp_strokes(rtdd_ctx *ctx, const rtdd_ramp_stroke *strokes , int count, uint8_t *edited, size_t editedPitch, "
            "uint8_t *scribble, size_t scribblePitch, const uint8_t *original, size_t originalPitch, int rows, int cols);") in code
    assert "int rtdd_ramp_polyline(const int *xy , int n, int radius, int brush, int label0, int label1, rtdd_ramp_stroke *out );" in code
    for words in ("N = 2 * (label0 * (dd - t) + label1 * t) + dd", "t = min(max(v.d, 0), dd)", "L = N / (2 * dd)", "round half up"):
        assert words in header, words


def test_the_python_wrapper_exposes_them():
    assert [n for n, _ in rt.RampStroke._fields_] == ["x0", "y0", "x1", "y1", "radius", "brush", "label0", "label1"]
    assert all(t is C.c_int for _, t in rt.RampStroke._fields_) and C.sizeof(rt.RampStroke) == 32
    assert {"rtdd_paint_ramp_strokes", "rtdd_ramp_polyline"} <= set(rt.C_ABI_SYMBOLS)
    assert callable(rt.Context.paint_ramp_strokes) and callable(rt.ramp_polyline)


# ---- rtdd_ramp_polyline through librtdd.so: host arithmetic, no device ----------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    rt.build()
    return rt.lib()


def _random_points(rng, n, span=400):
    pts = [(int(rng.integers(-span, span)), int(rng.integers(-span, span)))]
    for i in range(1, n):
        if i % 5 == 2:
            pts.append(pts[-1])                                       # a zero-length segment
        else:
            pts.append((int(np.clip(pts[-1][0] + rng.integers(-60, 61), -32768, 32767)), int(np.clip(pts[-1][1] + rng.integers(-60, 61), -32768, 32767))))
    return pts


def test_ramp_polyline_is_its_restatement(built):
    rng = np.random.default_rng(21)
    cases = 0
    for n in (1, 2, 3, 4, 7, 33, 300, 4097):
        for l0, l1 in ((0, 255), (255, 0), (40, 200), (17, 17), (3, 4), (int(rng.integers(0, 256)), int(rng.integers(0, 256)))):
            pts = _random_points(rng, n)
            radius, brush = int(rng.integers(0, 1025)), int(rng.integers(0, 2))
            got = rt.ramp_polyline(pts, radius, brush, l0, l1)
            assert got == rr.ramp_polyline(pts, radius, brush, l0, l1), (n, l0, l1)
            assert len(got) == max(n - 1, 1)
            labels = [got[0][6]] + [q[7] for q in got]
            assert all(a[7] == b[6] for a, b in zip(got[:-1], got[1:]))                     # neighbours share their vertex label
            assert all((a[2], a[3]) == (b[0], b[1]) for a, b in zip(got[:-1], got[1:]))
            assert labels[0] == l0                                                          # the ends are exact
            moved = any(p != pts[0] for p in pts)
            assert labels[-1] == (l1 if moved else l0)
            d = np.diff(labels)
            assert (d >= 0).all() if l1 >= l0 else (d <= 0).all()                           # monotone
            assert all(q[6] == q[7] for q in got if (q[0], q[1]) == (q[2], q[3]))           # a zero-length segment is a constant stamp
            cases += 1
    assert cases == 48
    # the domain's corners: the longest segments there are
    far = [(-32768, -32768), (32767, 32767), (-32768, 32767), (32767, -32768), (0, 0)]
    assert rt.ramp_polyline(far, 1024, 1, 0, 255) == rr.ramp_polyline(far, 1024, 1, 0, 255)


def test_ramp_polyline_of_one_point_and_of_no_length(built):
    assert rt.ramp_polyline([(5, -7)], 9, 1, 30, 200) == [(5, -7, 5, -7, 9, 1, 30, 30)]     # n == 1: one stamp, both labels label0
    same = [(12, 34)] * 5
    got = rt.ramp_polyline(same, 4, 0, 30, 200)                                             # S == 0: every label is label0
    assert got == [(12, 34, 12, 34, 4, 0, 30, 30)] * 4 == rr.ramp_polyline(same, 4, 0, 30, 200)


def test_ramp_polyline_refusals(built):
    L = built
    out = (rt.RampStroke * 5000)()

    def call(pts=((1, 2), (30, 40), (50, 45)), n=None, radius=5, brush=1, l0=10, l1=20, null_xy=False, null_out=False):
        flat = [v for p in pts for v in p]
        xy = (C.c_int * max(len(flat), 2))(*flat)
        return L.rtdd_ramp_polyline(None if null_xy else xy, C.c_int(len(pts) if n is None else n), C.c_int(radius), C.c_int(brush), C.c_int(l0), C.c_int(l1),
                                    None if null_out else out)
    refused = {
        "null xy": call(null_xy=True), "null out": call(null_out=True), "n == 0": call(n=0), "n < 0": call(n=-3), "n > 4097": call(pts=[(1, 1)] * 4098),
        "label0 256": call(l0=256), "label1 256": call(l1=256), "label0 erase": call(l0=-1), "label1 erase": call(l1=-1), "both erase": call(l0=-1, l1=-1),
        "label0 -2": call(l0=-2), "radius -1": call(radius=-1), "radius 1025": call(radius=1025), "brush 2": call(brush=2), "brush -1": call(brush=-1),
        "x too small": call(pts=((-32769, 0), (1, 1))), "x too large": call(pts=((0, 0), (32768, 1))), "y too small": call(pts=((0, 0), (1, -32769))),
        "y too large": call(pts=((0, 32768),)), "a bad point behind good ones": call(pts=((0, 0), (1, 1), (2, 2), (40000, 2))),
    }
    assert {k: v for k, v in refused.items() if v != 1} == {}
    assert call() == 0 and call(pts=[(1, 1)] * 4097) == 0 and call(pts=((-32768, 32767),), radius=1024, l0=0, l1=255) == 0
    assert call(radius=0, brush=0, l0=255, l1=0) == 0
    with pytest.raises(rt.RtddError):
        rt.ramp_polyline([(0, 0), (1, 1)], 5, 1, -1, 7)
