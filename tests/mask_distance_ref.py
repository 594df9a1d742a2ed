"""Restatements of rtdd_mask_distance, rtdd_refine_mask and rtdd_lift_layer_matte (include/rtdd.h) for the tests.  Three routes to E, the
squared Euclidean distance of a pixel to the nearest pixel of the other class, that share no code and know nothing of the kernels (no
tiles, no bands, no reach): `e_brute`, a per-pixel walk in Python integers; `e_scipy`, scipy's distance transform asked for the nearest
pixel's INDICES, the squared distance formed from them in integers; `e_separable`, numpy, a column pass and a row pass over whole arrays.
E is int64 with INF where the other class is empty.  On top: the signed map with the reach's cut-off, the four refine rules (the feather in
numpy float32, whose sqrt and / are correctly rounded) and the matte lift.  Test infrastructure."""
import math

import numpy as np

F = np.float32
INF = np.int64(1) << 40                 # E where the other class is empty: above every image's rows^2 + cols^2
FAR = 0x7FFFFFFF                        # RTDD_DISTANCE_FAR
GROW, SHRINK, OUTLINE, FEATHER = range(4)


def selected(mask, select):
    return (mask != 0) if select == 0 else (mask == select)


def refine(select=0, op=GROW, inner2=0, outer2=0, lo=0.0, hi=0.0):
    """The fields of rtdd_mask_refine as a dict; the floats are rounded to f32 as the struct holds them."""
    return dict(select=int(select), op=int(op), inner2=int(inner2), outer2=int(outer2), lo=float(F(lo)), hi=float(F(hi)))


# ---- E, three ways ---------------------------------------------------------------------------------------------------------------------

def e_brute(sel):
    """Per pixel, the minimum over every pixel of the other class, in Python integers."""
    rows, cols = sel.shape
    pts = {True: [(y, x) for y in range(rows) for x in range(cols) if sel[y, x]],
           False: [(y, x) for y in range(rows) for x in range(cols) if not sel[y, x]]}
    out = np.empty((rows, cols), np.int64)
    for y in range(rows):
        for x in range(cols):
            other = pts[not sel[y, x]]
            out[y, x] = min(((y - qy) ** 2 + (x - qx) ** 2 for qy, qx in other), default=int(INF))
    return out


def e_scipy(sel):
    """scipy.ndimage.distance_transform_edt's nearest-pixel indices; the squared distance from them in integers."""
    from scipy import ndimage
    rows, cols = sel.shape
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.int64)
    out = np.full((rows, cols), INF, np.int64)
    for cls in (True, False):                                               # pixels of class `cls`: their nearest pixel of the other class
        mine = sel == cls
        if mine.all() or not mine.any():
            continue
        iy, ix = ndimage.distance_transform_edt(mine, return_distances=False, return_indices=True)
        d2 = (yy - iy) ** 2 + (xx - ix) ** 2
        out[mine] = d2[mine]
    return out


def _vertical(target):
    """Per pixel the distance to the nearest True pixel of `target` in its own column (INF: none)."""
    rows, cols = target.shape
    big = np.int64(1) << 20
    up = np.full((rows, cols), big, np.int64); down = up.copy()
    run = np.full(cols, big, np.int64)
    for y in range(rows):
        run = np.where(target[y], 0, run + 1); up[y] = run
    run = np.full(cols, big, np.int64)
    for y in range(rows - 1, -1, -1):
        run = np.where(target[y], 0, run + 1); down[y] = run
    g = np.minimum(up, down)
    return np.where(g >= big, INF, g)


def _to_class(target):
    """Per pixel the squared distance to the nearest True pixel of `target`: min over columns x' of (x - x')^2 + g(x', y)^2."""
    rows, cols = target.shape
    g = _vertical(target)
    g2 = np.where(g >= INF, INF, g * g)
    out = np.full((rows, cols), INF, np.int64)
    x = np.arange(cols, dtype=np.int64)
    for xp in range(cols):
        col = g2[:, xp]
        if (col >= INF).all():
            continue
        out = np.minimum(out, (x[None, :] - xp) ** 2 + col[:, None])
    return np.minimum(out, INF)


def e_separable(sel):
    return np.where(sel, _to_class(~sel), _to_class(sel))


# ---- the calls -------------------------------------------------------------------------------------------------------------------------

def distance(E, sel, reach):
    """rtdd_mask_distance's dist2 from the unbounded E: signed, FAR beyond the reach."""
    v = np.where(E <= reach * reach, E, FAR)
    return np.where(sel, -v, v).astype(np.int32)


def reach_of(R):
    """The reach the host derives from a refine (a dict)."""
    if R["op"] == FEATHER:
        return math.ceil(max(abs(R["lo"]), abs(R["hi"])) + 0.5)
    most = {GROW: R["outer2"], SHRINK: R["inner2"]}.get(R["op"], max(R["inner2"], R["outer2"]))
    r = 1
    while r * r < most:
        r += 1
    return r


def feather_byte(E, sel, lo, hi):
    """The feather's byte per pixel from E (int64, INF allowed), one f32 operation per line of the header."""
    lo, hi = F(lo), F(hi)
    finite = E < INF
    t = np.sqrt(np.where(finite, E, 1).astype(F))
    s = np.where(sel, F(0.5) - t, t - F(0.5)).astype(F)
    with np.errstate(over="ignore", divide="ignore"):
        u = ((hi - s) / (hi - lo)).astype(F)
    u = np.minimum(np.maximum(u, F(0)), F(1)).astype(F)
    b = (u * F(255) + F(0.5)).astype(F).astype(np.int32)
    return np.where(finite, b, np.where(sel, 255, 0)).astype(np.uint8)


def refine_mask(E, sel, R):
    """rtdd_refine_mask: the rule applied to the unbounded E."""
    op = R["op"]
    if op == GROW:
        on = sel | (E <= R["outer2"])
    elif op == SHRINK:
        on = sel & (E > R["inner2"])
    elif op == OUTLINE:
        on = (sel & (E <= R["inner2"])) | (~sel & (E <= R["outer2"]))
    else:
        return feather_byte(E, sel, R["lo"], R["hi"])
    return np.where(on, 255, 0).astype(np.uint8)


def refine_from_distance(dist2, R):
    """The same rule from rtdd_mask_distance's output at the derived reach (FAR is an E beyond it)."""
    sel = dist2 < 0
    a = np.abs(dist2.astype(np.int64))
    return refine_mask(np.where(a == FAR, INF, a), sel, R)


def lift_matte(orig, alpha, x, y, srows, scols):
    """rtdd_lift_layer_matte: texel (u, v) is (B, G, R, a) of image pixel (x + u, y + v); zero where a == 0 or outside."""
    rows, cols = alpha.shape
    sprite = np.zeros((srows, scols, 4), np.uint8)
    v0, v1 = max(0, -y), min(srows, rows - y)
    u0, u1 = max(0, -x), min(scols, cols - x)
    if v0 < v1 and u0 < u1:
        a = alpha[y + v0:y + v1, x + u0:x + u1]
        sprite[v0:v1, u0:u1, :3] = np.where((a != 0)[..., None], orig[y + v0:y + v1, x + u0:x + u1], 0)
        sprite[v0:v1, u0:u1, 3] = a
    return sprite


# ---- the masks the tests share ---------------------------------------------------------------------------------------------------------

def single_pixels(rows, cols, points, code=7):
    m = np.zeros((rows, cols), np.uint8)
    for y, x in points:
        if 0 <= y < rows and 0 <= x < cols:
            m[y, x] = code
    return m
