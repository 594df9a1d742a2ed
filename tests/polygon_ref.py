"""rtdd_fill_polygon restated (include/rtdd.h, "a filled polygon"): test infrastructure.

A contour V is a list of (x, y) vertices, a fill the 7-tuple (rule, ax0, ay0, ax1, ay1, label0, label1) of rtdd_fill.  `winding_at` and
`on_boundary` are the header's rule in Python integers, one pixel at a time (arbitrary precision: the yardstick); `coverage` and
`fill_polygon` are the same rule in numpy int64 over the contour's bounding box clipped to the image (|cr| < 2^34, dd < 2^35, N < 2^45 on
the documented domain: nothing overflows; tests/test_fill_polygon_cpu.py pins them against the yardstick, the domain's corners
included), the label by ramp_ref.label_at's formula.  `tile_classes` and `fill_polygon_tiled` restate how the kernel's 64 x 16 tiles
classify the edges (nothing / a per-row base winding / live) and are pinned against the plain rule in the same file: the benchmark
counts its uniform tiles with the former."""
import numpy as np

import ramp_ref as rr

FILL_NONZERO, FILL_EVEN_ODD = 0, 1
STROKE_ERASE = -1
TILE_W, TILE_H = 64, 16


def _edges(V):
    V = [(int(x), int(y)) for x, y in V]
    return [(V[i], V[(i + 1) % len(V)]) for i in range(len(V))]


def winding_at(px, py, V):
    """The winding number of pixel (px, py): Python integers, the header's formulas as they stand."""
    px, py, w = int(px), int(py), 0
    for (ax, ay), (bx, by) in _edges(V):
        cr = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
        if ay <= py < by and cr > 0:
            w += 1
        if by <= py < ay and cr < 0:
            w -= 1
    return w


def on_boundary(px, py, V):
    px, py = int(px), int(py)
    for (ax, ay), (bx, by) in _edges(V):
        cr = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
        if cr == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return True
    return False


def covered_at(px, py, V, rule):
    w = winding_at(px, py, V)
    return on_boundary(px, py, V) or (w % 2 != 0 if rule == FILL_EVEN_ODD else w != 0)


def label_at(px, py, fill):
    """The label a painting fill gives a covered pixel: ramp_ref.label_at with the axis as the segment."""
    _, ax0, ay0, ax1, ay1, l0, l1 = (int(v) for v in fill)
    return l0 if l0 == l1 else rr.label_at(px, py, (ax0, ay0, ax1, ay1, 0, 0, l0, l1))


def box(V, rows, cols):
    """(xa, ya, xb, yb): the contour's bounding box clipped to the image, inclusive (None when it misses the image)."""
    xs, ys = [int(x) for x, _ in V], [int(y) for _, y in V]
    xa, xb, ya, yb = max(min(xs), 0), min(max(xs), cols - 1), max(min(ys), 0), min(max(ys), rows - 1)
    return None if xa > xb or ya > yb else (xa, ya, xb, yb)


def windings(V, rows, cols):
    """(ya, xa, w, on) over the clipped bounding box: the winding number (int64) and the boundary mask of every pixel (None outside)."""
    b = box(V, rows, cols)
    if b is None:
        return None
    xa, ya, xb, yb = b
    px = np.arange(xa, xb + 1, dtype=np.int64)[None, :]
    py = np.arange(ya, yb + 1, dtype=np.int64)[:, None]
    w = np.zeros((yb - ya + 1, xb - xa + 1), np.int64)
    on = np.zeros(w.shape, bool)
    for (ax, ay), (bx, by) in _edges(V):
        cr = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
        w += ((ay <= py) & (py < by) & (cr > 0)).astype(np.int64)
        w -= ((by <= py) & (py < ay) & (cr < 0)).astype(np.int64)
        on |= (cr == 0) & (min(ax, bx) <= px) & (px <= max(ax, bx)) & (min(ay, by) <= py) & (py <= max(ay, by))
    return ya, xa, w, on


def max_abs_cr(V, rows, cols):
    """The largest |cr| any pixel of the clipped bounding box sees on any edge (cr is affine: the box's corners suffice)."""
    xa, ya, xb, yb = box(V, rows, cols)
    return max(abs((bx - ax) * (py - ay) - (px - ax) * (by - ay)) for (ax, ay), (bx, by) in _edges(V) for px in (xa, xb) for py in (ya, yb))


def coverage(V, rule, rows, cols):
    """(ya, xa, mask) of the covered pixels over the clipped bounding box (None when the contour misses the image)."""
    hit = windings(V, rows, cols)
    if hit is None:
        return None
    ya, xa, w, on = hit
    return ya, xa, on | ((w & 1) != 0 if rule == FILL_EVEN_ODD else w != 0)


def _write(fill, edited, scribble, original, ya, xa, m):
    _, ax0, ay0, ax1, ay1, l0, l1 = (int(v) for v in fill)
    e = edited[ya:ya + m.shape[0], xa:xa + m.shape[1]]
    s = scribble[ya:ya + m.shape[0], xa:xa + m.shape[1]]
    if l0 == STROKE_ERASE:
        assert l1 == STROKE_ERASE
        e[m] = original[ya:ya + m.shape[0], xa:xa + m.shape[1]][m]
        s[m] = 0
        return
    dx, dy = ax1 - ax0, ay1 - ay0
    dd = dx * dx + dy * dy
    if dd == 0 or l0 == l1:
        lab = np.full(m.shape, l0, np.int64)
    else:
        px = np.arange(xa, xa + m.shape[1], dtype=np.int64)[None, :]
        py = np.arange(ya, ya + m.shape[0], dtype=np.int64)[:, None]
        t = np.clip((px - ax0) * dx + (py - ay0) * dy, 0, dd)
        lab = (2 * (l0 * (dd - t) + l1 * t) + dd) // (2 * dd)
    e[m] = lab[m].astype(np.uint8)[:, None]
    s[m] = 255


def fill_polygon(V, fill, edited, scribble, original=None):
    """rtdd_fill_polygon in place on edited [rows, cols, 3] and scribble [rows, cols]; returns the number of covered pixels."""
    if len(V) == 0:
        return 0
    rows, cols = scribble.shape
    hit = coverage(V, int(fill[0]), rows, cols)
    if hit is None:
        return 0
    ya, xa, m = hit
    _write(fill, edited, scribble, original, ya, xa, m)
    return int(m.sum())


# ---- the kernel's tiles restated -----------------------------------------------------------------------------------------------------
def tile_classes(V, rows, cols):
    """For every 64 x 16 tile of the launch (the clipped bounding box, its left edge rounded down to a multiple of 64), in row-major order:
    (tx0, ty0, tx1, ty1, base, live) -- base the 16 per-row windings from the edges wholly right of the tile, live the edges whose closed
    box meets it.  Empty when the contour misses the image."""
    b = box(V, rows, cols)
    if b is None:
        return []
    xa, ya, xb, yb = b
    xa &= ~63
    out = []
    for ty0 in range(ya, yb + 1, TILE_H):
        for tx0 in range(xa, xb + 1, TILE_W):
            tx1, ty1 = min(tx0 + TILE_W - 1, xb), min(ty0 + TILE_H - 1, yb)
            base, live = [0] * TILE_H, []
            for (ax, ay), (bx, by) in _edges(V):
                xmin, xmax, ymin, ymax = min(ax, bx), max(ax, bx), min(ay, by), max(ay, by)
                if ymin > ty1 or ymax < ty0 or xmax < tx0:
                    continue
                if xmin <= tx1:
                    live.append(((ax, ay), (bx, by)))
                elif ay != by:
                    for y in range(max(ymin, ty0), min(ymax - 1, ty1) + 1):
                        base[y - ty0] += 1 if by > ay else -1
            out.append((tx0, ty0, tx1, ty1, base, live))
    return out


def fill_polygon_tiled(V, fill, edited, scribble, original=None):
    """fill_polygon computed the kernel's way, tile by tile: cr at the tile's origin plus the pixel's affine part; returns (tiles,
    tiles without a live edge, of those the ones that store nothing)."""
    rows, cols = scribble.shape
    rule = int(fill[0])
    tiles = tile_classes(V, rows, cols)
    uniform = silent = 0
    for tx0, ty0, tx1, ty1, base, live in tiles:
        h, wd = ty1 - ty0 + 1, tx1 - tx0 + 1
        ry = np.arange(h, dtype=np.int64)[:, None]
        rx = np.arange(wd, dtype=np.int64)[None, :]
        w = np.array(base[:h], np.int64)[:, None].repeat(wd, 1)
        on = np.zeros((h, wd), bool)
        for (ax, ay), (bx, by) in live:
            dxe, dye = bx - ax, by - ay
            cr = dxe * (ty0 - ay) - (tx0 - ax) * dye + dxe * ry - dye * rx
            y, x = ty0 + ry, tx0 + rx
            w += ((ay <= y) & (y < by) & (cr > 0)).astype(np.int64)
            w -= ((by <= y) & (y < ay) & (cr < 0)).astype(np.int64)
            on |= (cr == 0) & (min(ax, bx) <= x) & (x <= max(ax, bx)) & (min(ay, by) <= y) & (y <= max(ay, by))
        m = on | ((w & 1) != 0 if rule == FILL_EVEN_ODD else w != 0)
        if not live:
            uniform += 1
            silent += int(not m.any())
            assert all((m[r] == m[r, 0]).all() for r in range(h))
        if m.any():
            _write(fill, edited, scribble, original, ty0, tx0, m)
    return len(tiles), uniform, silent


# ---- cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------------
PENTAGRAM = [(20, 6), (31, 39), (3, 18), (37, 18), (9, 39)]
TRAPEZOID = [(14, 6), (25, 6), (37, 44), (2, 44)]
RECTANGLE = [(4, 2), (8, 2), (8, 45), (4, 45)]


def constant(label, rule=FILL_NONZERO):
    return (rule, 0, 0, 0, 0, label, label)


def erase(rule=FILL_NONZERO):
    return (rule, 0, 0, 0, 0, STROKE_ERASE, STROKE_ERASE)


def random_contour(rng, rows, cols, n, margin=20):
    """n vertices from -margin to margin beyond the image; every third contour repeats a vertex, every fourth has a horizontal and a
    vertical edge."""
    V = [(int(rng.integers(-margin, cols + margin)), int(rng.integers(-margin, rows + margin))) for _ in range(n)]
    k = int(rng.integers(0, 12))
    if n >= 3 and k % 3 == 0:
        V[n // 2] = V[0]
    if n >= 4 and k % 4 == 1:
        V[1] = (V[1][0], V[0][1])
        V[2] = (V[1][0], V[2][1])
    return V


def random_fill(rng, rows, cols, kind, rule):
    """kind 0: constant, 1: ramp (an axis through the image, sometimes beyond it), 2: erase."""
    if kind == 2:
        return erase(rule)
    if kind == 0:
        return constant(int(rng.integers(0, 256)), rule)
    ax0, ay0, ax1, ay1 = (int(rng.integers(-30, cols + 30)), int(rng.integers(-30, rows + 30)), int(rng.integers(-30, cols + 30)), int(rng.integers(-30, rows + 30)))
    return (rule, ax0, ay0, ax1, ay1, int(rng.integers(0, 256)), int(rng.integers(0, 256)))


def scaled(V, fx, fy, ox=0, oy=0):
    return [(ox + x * fx, oy + y * fy) for x, y in V]


def spiky_ring(n, cx, cy, r_in, r_out):
    """n vertices alternating between two radii: a star whose spikes cross every tile of its box."""
    out = []
    for i in range(n):
        a = 2 * np.pi * i / n
        r = r_out if i % 2 == 0 else r_in
        out.append((int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))))
    return out


def wobbly_circle(n, cx, cy, r, wobble=0.06, waves=9):
    out = []
    for i in range(n):
        a = 2 * np.pi * i / n
        rr_ = r * (1 + wobble * np.sin(waves * a))
        out.append((int(round(cx + rr_ * np.cos(a))), int(round(cy + rr_ * np.sin(a)))))
    return out


# tile borders of a 37 x 150 image whose launch starts at x = 0: x = 63 | 64, 127 | 128; y = 15 | 16, 31 | 32
BORDER_CONTOURS = {
    "vertices on tile borders": [(63, 15), (128, 16), (127, 32), (64, 31)],
    "edges along tile borders": [(64, 16), (127, 16), (127, 31), (64, 31)],
    "edges one pixel inside the borders": [(63, 15), (128, 15), (128, 32), (63, 32)],
    "repeated vertices": [(10, 5), (10, 5), (140, 5), (140, 30), (140, 30), (140, 30), (70, 33), (10, 5), (20, 30)],
    "pentagram across the tiles": scaled(PENTAGRAM, 4, 1, -8, -4),
    # a "C" open to the right whose back reaches to x = 70 and whose opening is exactly the second tile row (y 16..31): there tile 0 has no
    # live edge and a base winding of +-1 (the back's inner edge lies wholly right of it), tile 2 has no live edge and winding 0
    "a concave C": [(-10, -9), (149, -9), (149, 15), (70, 15), (70, 32), (149, 32), (149, 60), (-10, 60)],
    "the C backwards": [(-10, -9), (149, -9), (149, 15), (70, 15), (70, 32), (149, 32), (149, 60), (-10, 60)][::-1],
    "twice round (w = 2)": [(5, 2), (145, 2), (145, 35), (5, 35), (5, 2), (145, 2), (145, 35), (5, 35)],
}

M, P = -32768, 32767
# the domain's corners against a 2 x 32768 and a 32768 x 2 image: cr passes 2^31 there and each of its two products 2^32
EXTREME_CONTOURS = [
    [(M, M), (P, P), (P, M)],
    [(M, M), (P, P), (M, P)],
    [(M, P), (P, M), (P, P)],
    [(M, M), (P, M), (P, P), (M, P)],
    [(M, M), (P, P)],
    [(M, M), (P, 1), (P, M)],
    [(M, M), (1, P), (M, P)],
    [(M, M), (P, P), (P, M), (M, P)],
    [(0, M), (P, 1), (3, P), (M, 0)],
]
EXTREME_AXES = [(M, M, P, P), (P, M, M, P), (M, 0, P, 1), (0, M, 1, P), (M, M, 40, 1), (P, P, 0, 0)]
