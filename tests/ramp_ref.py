"""rtdd_paint_ramp_strokes and rtdd_ramp_polyline restated (include/rtdd.h, "depth-ramp strokes"): test infrastructure.

A ramp stroke is the 8-tuple (x0, y0, x1, y1, radius, brush, label0, label1) of rtdd_ramp_stroke.  `label_at` is the header's label rule
in Python integers, one pixel at a time (arbitrary precision: the yardstick); `paint_ramp_strokes` is the same rule in numpy int64 over
strokes_ref.coverage's box (inside it |v| and |d| stay below 2^17, dd below 2^35 and N below 2^45: nothing overflows; the CPU tests pin
it against `label_at`, the domain's corners included); `ramp_polyline` is the arc-length rule in Python floats."""
import math

import numpy as np

import strokes_ref as sr

STROKE_ERASE = sr.STROKE_ERASE


def label_at(px, py, stroke):
    """The label a painting ramp stroke gives pixel (px, py) (whether it covers it is strokes_ref.covers' business)."""
    x0, y0, x1, y1 = (int(v) for v in stroke[:4])
    l0, l1 = int(stroke[6]), int(stroke[7])
    dx, dy = x1 - x0, y1 - y0
    dd = dx * dx + dy * dy
    if dd == 0:
        return l0
    t = min(max((int(px) - x0) * dx + (int(py) - y0) * dy, 0), dd)
    return (2 * (l0 * (dd - t) + l1 * t) + dd) // (2 * dd)


def paint_ramp_strokes(strokes, edited, scribble, original=None):
    """The ramp strokes in order, in place on edited [rows, cols, 3] and scribble [rows, cols]: the last stroke covering a pixel decides it."""
    rows, cols = scribble.shape
    for q in strokes:
        hit = sr.coverage(rows, cols, q)
        if hit is None:
            continue
        ya, xa, m = hit
        e = edited[ya:ya + m.shape[0], xa:xa + m.shape[1]]
        s = scribble[ya:ya + m.shape[0], xa:xa + m.shape[1]]
        x0, y0, x1, y1 = (int(v) for v in q[:4])
        l0, l1 = int(q[6]), int(q[7])
        if l0 == STROKE_ERASE:
            assert l1 == STROKE_ERASE
            e[m] = original[ya:ya + m.shape[0], xa:xa + m.shape[1]][m]
            s[m] = 0
            continue
        dx, dy = x1 - x0, y1 - y0
        dd = dx * dx + dy * dy
        if dd == 0:
            lab = np.full(m.shape, l0, np.int64)
        else:
            px = np.arange(xa, xa + m.shape[1], dtype=np.int64)[None, :]
            py = np.arange(ya, ya + m.shape[0], dtype=np.int64)[:, None]
            t = np.clip((px - x0) * dx + (py - y0) * dy, 0, dd)
            lab = (2 * (l0 * (dd - t) + l1 * t) + dd) // (2 * dd)
        e[m] = lab[m].astype(np.uint8)[:, None]
        s[m] = 255


# ---- cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------------
EXTREMES = [(-32768, -32768, 32767, 32767), (32767, -32768, -32768, 32767)]
# exact half ties: horizontal segments of even length with an odd label difference (the middle pixel lies exactly between two labels)
HALF_TIES = [(0, 0, 2, 0, 1, sr.BRUSH_SQUARE, 0, 1), (3, 5, 13, 5, 5, sr.BRUSH_ROUND, 10, 17), (40, 30, 4, 30, 3, sr.BRUSH_SQUARE, 200, 1),
             (2, 40, 30, 40, 7, sr.BRUSH_ROUND, 255, 0)]


def extreme_strokes():
    """Single strokes along the domain's two diagonals, radius 1024, labels both ways; and the same segments shifted so that a 67 x 45
    image lies across the stroke's middle and sees several labels (N near its bound of 2^45)."""
    out = []
    for (x0, y0, x1, y1) in EXTREMES:
        for l0, l1 in ((0, 255), (255, 0)):
            for brush in (sr.BRUSH_SQUARE, sr.BRUSH_ROUND):
                out.append((x0, y0, x1, y1, 1024, brush, l0, l1))
    # a diagonal that ends inside the image: the far end's labels change every few pixels there ... and one whose short length makes
    # every pixel another label
    out += [(-32768, -32768, 40, 60, 1024, sr.BRUSH_ROUND, 0, 255), (32767, -32768, 5, 40, 1024, sr.BRUSH_SQUARE, 255, 0),
            (-32768, 32767, 30, 10, 1024, sr.BRUSH_SQUARE, 7, 250), (-300, -200, 340, 260, 1024, sr.BRUSH_ROUND, 0, 255),
            (200, -150, -160, 190, 1024, sr.BRUSH_SQUARE, 255, 0)]
    return out


def ramp_polyline(points, radius, brush, label0, label1):
    """rtdd_ramp_polyline: the points [(x, y), ...] as max(n - 1, 1) ramp strokes, the labels spread by arc length (doubles, every operation
    rounded on its own -- Python floats are)."""
    pts = [(int(x), int(y)) for x, y in points]
    n = len(pts)
    if n == 1:
        return [(pts[0][0], pts[0][1], pts[0][0], pts[0][1], radius, brush, label0, label0)]
    s = [0.0]
    for (xa, ya), (xb, yb) in zip(pts[:-1], pts[1:]):
        s.append(s[-1] + math.sqrt(float((xb - xa) ** 2 + (yb - ya) ** 2)))
    S = s[-1]
    lab = [int(math.floor(label0 + (label1 - label0) * (si / S) + 0.5)) if S > 0 else label0 for si in s]
    return [(pts[i][0], pts[i][1], pts[i + 1][0], pts[i + 1][1], radius, brush, lab[i], lab[i + 1]) for i in range(n - 1)]
