"""rtdd_paint_strokes and rtdd_pyramid_annotation_rebuild restated (include/rtdd.h, "brush strokes and an eraser"): test infrastructure.

A stroke is the 7-tuple (x0, y0, x1, y1, radius, brush, label) of rtdd_stroke.  `covers` is the header's coverage rule in Python integers,
one pixel at a time (arbitrary precision: the yardstick); `coverage` is the same rule in numpy over the stroke's bounding box clipped to
the image, arranged so that no int64 / uint64 product overflows on the documented domain (tests/test_strokes_cpu.py pins it against
`covers`, the domain's corners included)."""
import numpy as np

BRUSH_SQUARE, BRUSH_ROUND = 0, 1
STROKE_ERASE = -1


def covers(px, py, stroke):
    """Does the stroke cover pixel (px, py)?  Python integers, the header's formulas as they stand."""
    x0, y0, x1, y1, radius, brush = (int(v) for v in stroke[:6])
    px, py = int(px), int(py)
    dx, dy, vx, vy, h = x1 - x0, y1 - y0, px - x0, py - y0, radius // 2
    cross = dx * vy - dy * vx
    if brush == BRUSH_SQUARE:
        return (min(x0, x1) - h <= px <= max(x0, x1) + h and min(y0, y1) - h <= py <= max(y0, y1) + h
                and abs(cross) <= h * (abs(dx) + abs(dy)))
    t, dd = vx * dx + vy * dy, dx * dx + dy * dy
    if t <= 0:
        return 4 * (vx * vx + vy * vy) <= radius * radius
    if t >= dd:
        return 4 * ((px - x1) ** 2 + (py - y1) ** 2) <= radius * radius
    return (2 * cross) ** 2 <= radius * radius * dd


def coverage(rows, cols, stroke):
    """(ya, xa, mask): the pixels the stroke covers, as a boolean array over rows ya.., columns xa.. (None when it misses the image).
    Only the stroke's bounding box grown by radius // 2 is looked at (a round brush reaches no further either: a covered pixel has integer
    coordinates within radius / 2 of the segment), which keeps |v| and |d| below 2^17 and every product below 2^35; the one square that can
    pass 2^63, (2 cross)^2, is formed only where 2 |cross| < 2^32 -- beyond that it exceeds radius^2 |d|^2 <= 2^54 anyway."""
    x0, y0, x1, y1, radius, brush = (int(v) for v in stroke[:6])
    h = radius // 2
    xa, xb = max(min(x0, x1) - h, 0), min(max(x0, x1) + h, cols - 1)
    ya, yb = max(min(y0, y1) - h, 0), min(max(y0, y1) + h, rows - 1)
    if xa > xb or ya > yb:
        return None
    px = np.arange(xa, xb + 1, dtype=np.int64)[None, :]
    py = np.arange(ya, yb + 1, dtype=np.int64)[:, None]
    dx, dy = x1 - x0, y1 - y0
    vx, vy = px - x0, py - y0
    ac = np.abs(dx * vy - dy * vx)
    if brush == BRUSH_SQUARE:
        return ya, xa, ac <= h * (abs(dx) + abs(dy))
    t, dd, r2 = vx * dx + vy * dy, dx * dx + dy * dy, radius * radius
    head = 4 * (vx * vx + vy * vy) <= r2
    tail = 4 * ((px - x1) ** 2 + (py - y1) ** 2) <= r2
    c2 = 2 * ac
    small = c2 < (1 << 32)
    c2u = np.where(small, c2, 0).astype(np.uint64)
    body = small & (c2u * c2u <= np.uint64(r2 * dd))
    return ya, xa, np.where(t <= 0, head, np.where(t >= dd, tail, body))


def paint_strokes(strokes, edited, scribble, original=None):
    """The strokes in order, in place on edited [rows, cols, 3] and scribble [rows, cols]: the last stroke covering a pixel decides it."""
    rows, cols = scribble.shape
    for q in strokes:
        hit = coverage(rows, cols, q)
        if hit is None:
            continue
        ya, xa, m = hit
        e = edited[ya:ya + m.shape[0], xa:xa + m.shape[1]]
        s = scribble[ya:ya + m.shape[0], xa:xa + m.shape[1]]
        if int(q[6]) == STROKE_ERASE:
            e[m] = original[ya:ya + m.shape[0], xa:xa + m.shape[1]][m]
            s[m] = 0
        else:
            e[m] = int(q[6])
            s[m] = 255


def rebuild(cascade):
    """rtdd_pyramid_annotation_rebuild on a cascade_ref.Cascade: the coarse annotation levels as after creation (all zero); the next
    `estimate` then down-samples into them as usual.  The depth pyramid (the warm start) is left alone."""
    for l in range(1, cascade.P):
        cascade.scribble[l][...] = 0
        cascade.edited[l][...] = 0


def stamps_along(polyline, radius):
    """The rtdd_paint_image stamps a host needs to leave no gap along a polyline with a brush of half-width radius // 2: one per pixel
    step of the longer axis of every segment (consecutive square stamps of side 2 h + 1 >= 1 then always touch)."""
    out = []
    for (x0, y0), (x1, y1) in zip(polyline[:-1], polyline[1:]):
        n = max(abs(x1 - x0), abs(y1 - y0), 1)
        for i in range(n + 1):
            p = (x0 + (x1 - x0) * i // n, y0 + (y1 - y0) * i // n)
            if not out or out[-1] != p:
                out.append(p)
    return out
