"""Two restatements of rtdd_simulate_ambient_occlusion (include/rtdd.h) for the tests, built on relight_ref.py for d', shade and k_c:
`ambient` / `occluded` in vectorised numpy float32 with a loop over the directions and the steps, and `ambient_literal` /
`occluded_literal`, per-pixel loops over the header's lines.  Every operation is one f32 operation rounded once, in the header's order;
the tables inv_j[k] are computed in double and rounded once, as the header has the host do.  Neither knows about the kernel.  The
vectorised one reads a position outside the image as a height of minus infinity (the image is convex and a direction a straight line:
once outside, a march stays outside, and minus infinity never wins a maximum); the literal one ends the march there, as the rule is
written.  Neither uses the header's early exit.  `rows=(y0, y1)` restates a band of rows only, on the whole map.  Test infrastructure."""
import math

import numpy as np

from relight_ref import F, channel_gains, clamp_depth, shade

SHADE, MAP = 0, 1
DIRECTIONS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def occlusion(mode=SHADE, directions=8, radius=16, relief=1.0, bias=0.0, strength=1.0):
    """The fields of rtdd_ambient_occlusion as a dict; the floats are rounded to f32 as the struct holds them."""
    return dict(mode=int(mode), directions=int(directions), radius=int(radius), relief=float(F(relief)), bias=float(F(bias)),
                strength=float(F(strength)))


def inv_step(j, k):
    """inv_j[k]: (float)(1.0 / (double)k) on the axes, (float)(1.0 / ((double)k * sqrt(2.0))) on the diagonals."""
    return F(1.0 / float(k)) if j % 2 == 0 else F(1.0 / (float(k) * math.sqrt(2.0)))


def _directions(A):
    assert A["directions"] in (4, 8)
    return range(0, 8, 8 // A["directions"])


def ambient(depth, A, rows=None):
    """ao (f32) of every pixel of the rows [y0, y1) (default: all), shape (y1 - y0, cols)."""
    dc = clamp_depth(np.asarray(depth, F))
    nrows, cols = dc.shape
    y0, y1 = rows if rows is not None else (0, nrows)
    r, bias = A["radius"], F(A["bias"])
    H = F(A["relief"]) * (F(255) - dc)
    Hp = np.full((nrows + 2 * r, cols + 2 * r), -np.inf, F)
    Hp[r:r + nrows, r:r + cols] = H
    h0 = H[y0:y1]
    s = None
    with np.errstate(invalid="raise"):                              # nothing produces a NaN
        for j in _directions(A):
            ux, uy = DIRECTIONS[j]
            tmax = np.zeros(h0.shape, F)
            for k in range(1, r + 1):
                hp = Hp[r + y0 + k * uy:r + y1 + k * uy, r + k * ux:r + k * ux + cols]
                rise = (hp - h0) - bias
                t = rise * inv_step(j, k)
                assert t.dtype == F
                np.maximum(tmax, t, out=tmax)
            occ = tmax / np.sqrt(F(1) + (tmax * tmax))
            s = occ if s is None else s + occ
        mean = s * F(1.0 / A["directions"])
        ao = F(1) - (F(A["strength"]) * mean)
    assert ao.dtype == F
    return ao


def _u8(v):
    assert v.dtype == F
    return v.astype(np.int32).astype(np.uint8)


def apply_ao(orig, ao, A, L=None, s=None):
    """The bytes from ao: the original darkened, the map, or (L: the light, s: relight's shade) relight with its ambient term occluded."""
    out = np.empty(ao.shape + (3,), np.uint8)
    if A["mode"] == MAP:
        assert L is None
        out[...] = _u8(F(255) * ao)[..., None]
    elif L is None:
        for c in range(3):
            out[..., c] = _u8(orig[..., c].astype(F) * ao)
    else:
        assert F(L["relief"]) == F(A["relief"])
        amb = F(L["ambient"]) * ao
        for c, k in enumerate(channel_gains(L)):
            out[..., c] = _u8(np.fmin(orig[..., c].astype(F) * (amb + (k * s)), F(255)))
    return out


def occluded(orig, depth, A, L=None, rows=None):
    """rtdd_simulate_ambient_occlusion's image (rows=None), or its rows [y0, y1)."""
    depth = np.asarray(depth, F)
    y0, y1 = rows if rows is not None else (0, depth.shape[0])
    s = shade(depth, L)[y0:y1] if L is not None else None
    return apply_ao(orig[y0:y1], ambient(depth, A, rows), A, L, s)


def ambient_literal(depth, A, occ_out=None):
    """The header's lines, one pixel at a time, every intermediate an np.float32 scalar.  occ_out: an f32 array (rows, cols, 8) that
    receives occ_j."""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape
    relief, bias, strength, r = F(A["relief"]), F(A["bias"]), F(A["strength"]), A["radius"]

    def height(x, y):
        d = depth[y, x]
        dp = F(0) if d != d else F(min(max(d, F(0)), F(255)))
        return F(relief * F(F(255) - dp))

    Hh = [[height(x, y) for x in range(cols)] for y in range(rows)]
    inv = [[None] + [inv_step(j, k) for k in range(1, r + 1)] for j in range(2)]
    ao = np.empty((rows, cols), F)
    for y in range(rows):
        for x in range(cols):
            h = Hh[y][x]
            s = None
            for j in _directions(A):
                ux, uy = DIRECTIONS[j]
                tmax = F(0)
                for k in range(1, r + 1):
                    px, py = x + k * ux, y + k * uy
                    if px < 0 or px >= cols or py < 0 or py >= rows:
                        break
                    rise = F(F(Hh[py][px] - h) - bias)
                    t = F(rise * inv[j % 2][k])
                    if t > tmax:
                        tmax = t
                occ = F(tmax / np.sqrt(F(F(1) + F(tmax * tmax))))
                if occ_out is not None:
                    occ_out[y, x, j] = occ
                s = occ if s is None else F(s + occ)
            mean = F(s * F(1.0 / A["directions"]))
            ao[y, x] = F(F(1) - F(strength * mean))
    return ao


def occluded_literal(orig, depth, A, L=None, ao=None):
    """The output lines of the header, one pixel at a time; ao: ambient_literal's (computed here when None)."""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape
    if ao is None:
        ao = ambient_literal(depth, A)
    out = np.empty((rows, cols, 3), np.uint8)
    if L is not None:
        assert A["mode"] == SHADE and F(L["relief"]) == F(A["relief"])
        s_all = shade(depth, L)                                   # relight's shade (pinned against its own literal loop by test_relight_cpu.py)
        amb0, ks = F(L["ambient"]), channel_gains(L)
    for y in range(rows):
        for x in range(cols):
            a = F(ao[y, x])
            for c in range(3):
                if A["mode"] == MAP:
                    v = F(F(255) * a)
                elif L is None:
                    v = F(F(orig[y, x, c]) * a)
                else:
                    v = F(min(F(F(orig[y, x, c]) * F(F(amb0 * a) + F(ks[c] * s_all[y, x]))), F(255)))
                out[y, x, c] = int(v)
    return out
