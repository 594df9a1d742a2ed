"""Two restatements of rtdd_simulate_relight (include/rtdd.h) for the tests: `relight` in vectorised numpy float32, and
`relight_literal`, a per-pixel loop over the formulas as the header states them.  Every operation is one f32 operation rounded once,
in the header's order; what the header computes on the host (the unit direction, invR2, the k_c) is computed in double here too.
Neither knows about the kernel.  Test infrastructure."""
import math

import numpy as np

DIRECTIONAL, POINT = 0, 1
F = np.float32


def light(kind=DIRECTIONAL, x=0.0, y=0.0, z=1.0, anchorDepth=0.0, anchorX=-1, anchorY=-1, radius=1.0, relief=1.0, ambient=0.0, diffuse=1.0,
          color=(255, 255, 255)):
    """The fields of rtdd_light as a dict (color = (b, g, r)); the floats are rounded to f32 as the struct holds them."""
    return dict(kind=int(kind), x=float(F(x)), y=float(F(y)), z=float(F(z)), anchorDepth=float(F(anchorDepth)), anchorX=int(anchorX),
                anchorY=int(anchorY), radius=float(F(radius)), relief=float(F(relief)), ambient=float(F(ambient)), diffuse=float(F(diffuse)),
                color=tuple(int(c) for c in color))


def clamp_depth(d):
    """d' = fminf(fmaxf(d, 0), 255) in f32: a NaN depth is 0."""
    return np.fmin(np.fmax(np.asarray(d, F), F(0)), F(255))


def unit_direction(L):
    """(lx, ly, lz): the unit vector of (x, y, z), normalised in double, each component rounded to f32."""
    x, y, z = L["x"], L["y"], L["z"]
    n = math.sqrt(((x * x) + (y * y)) + (z * z))
    return F(x / n), F(y / n), F(z / n)


def channel_gains(L):
    """k_c = (float)((double)diffuse * color_c / 255.0) for c of B, G, R."""
    return [F(L["diffuse"] * c / 255.0) for c in L["color"]]


def inv_r2(L):
    return F(1.0 / (L["radius"] * L["radius"]))


def anchor_depth(depth, L):
    return clamp_depth(depth[L["anchorY"], L["anchorX"]]) if L["anchorX"] >= 0 else F(L["anchorDepth"])


def shade(depth, L):
    """The f32 shade of every pixel."""
    dc = clamp_depth(depth)
    rows, cols = dc.shape
    xs, ys = np.arange(cols), np.arange(rows)
    gx = dc[:, np.minimum(xs + 1, cols - 1)] - dc[:, np.maximum(xs - 1, 0)]
    gy = dc[np.minimum(ys + 1, rows - 1), :] - dc[np.maximum(ys - 1, 0), :]
    relief = F(L["relief"])
    nx, ny = relief * gx, relief * gy
    nn = ((nx * nx) + (ny * ny)) + F(4)
    if L["kind"] == DIRECTIONAL:
        lx, ly, lz = unit_direction(L)
        dot = ((nx * lx) + (ny * ly)) + (F(2) * lz)
        s = np.fmax(dot, F(0)) / np.sqrt(nn)
    else:
        dA = anchor_depth(depth, L)
        Lz = (relief * (F(255) - dA)) + F(L["z"])
        vx = np.broadcast_to((F(L["x"]) - xs.astype(F))[None, :], dc.shape)
        vy = np.broadcast_to((F(L["y"]) - ys.astype(F))[:, None], dc.shape)
        vz = Lz - (relief * (F(255) - dc))
        vv = ((vx * vx) + (vy * vy)) + (vz * vz)
        dot = ((nx * vx) + (ny * vy)) + (F(2) * vz)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (np.fmax(dot, F(0)) / np.sqrt(nn * vv)) / (F(1) + (vv * inv_r2(L)))
        s = np.where(vv == 0, F(0), s)
    assert s.dtype == F
    return s


def apply_gain(orig, s, L):
    """out_c = (uchar) fminf(o_c * (ambient + (k_c * shade)), 255), truncated."""
    out = np.empty_like(orig)
    amb = F(L["ambient"])
    for c, k in enumerate(channel_gains(L)):
        v = np.fmin(orig[..., c].astype(F) * (amb + (k * s)), F(255))
        assert v.dtype == F
        out[..., c] = v.astype(np.int32).astype(np.uint8)
    return out


def relight(orig, depth, L):
    return apply_gain(orig, shade(np.asarray(depth, F), L), L)


def relight_literal(orig, depth, L):
    """The header's lines, one pixel at a time, every intermediate an np.float32 scalar."""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape

    def dp(x, y):
        d = depth[y, x]
        if d != d:
            return F(0)
        return F(min(max(d, F(0)), F(255)))

    relief, amb = F(L["relief"]), F(L["ambient"])
    ks = channel_gains(L)
    if L["kind"] == DIRECTIONAL:
        lx, ly, lz = unit_direction(L)
    else:
        dA = dp(L["anchorX"], L["anchorY"]) if L["anchorX"] >= 0 else F(L["anchorDepth"])
        Lz = F(F(relief * F(F(255) - dA)) + F(L["z"]))
        invR2 = inv_r2(L)
    out = np.empty_like(orig)
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                gx = F(dp(min(x + 1, cols - 1), y) - dp(max(x - 1, 0), y))
                gy = F(dp(x, min(y + 1, rows - 1)) - dp(x, max(y - 1, 0)))
                nx, ny = F(relief * gx), F(relief * gy)
                nn = F(F(F(nx * nx) + F(ny * ny)) + F(4))
                if L["kind"] == DIRECTIONAL:
                    dot = F(F(F(nx * lx) + F(ny * ly)) + F(F(2) * lz))
                    s = F(max(dot, F(0)) / np.sqrt(nn))
                else:
                    vx, vy = F(F(L["x"]) - F(x)), F(F(L["y"]) - F(y))
                    vz = F(Lz - F(relief * F(F(255) - dp(x, y))))
                    vv = F(F(F(vx * vx) + F(vy * vy)) + F(vz * vz))
                    dot = F(F(F(nx * vx) + F(ny * vy)) + F(F(2) * vz))
                    if vv == 0:
                        s = F(0)
                    else:
                        s = F(F(max(dot, F(0)) / np.sqrt(F(nn * vv))) / F(F(1) + F(vv * invR2)))
                for c in range(3):
                    v = F(F(orig[y, x, c]) * F(amb + F(ks[c] * s)))
                    out[y, x, c] = int(min(v, F(255)))
    return out
