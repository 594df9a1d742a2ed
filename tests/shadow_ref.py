"""Two restatements of rtdd_simulate_relight_shadowed (include/rtdd.h) for the tests, built on relight_ref.py: `relight_shadowed` in
vectorised numpy float32 with a loop over the steps k, and `relight_shadowed_literal`, a per-pixel loop over the header's lines.  Every
operation is one f32 operation rounded once, in the header's order.  Neither knows about the kernel: the vectorised one only drops a
pixel from its working set when its march has ended (the image left, k == n) or when q == 1, which no later q_k <= 1 can raise; it
does not use the header's other freedom (the ray above relief * 255).  `rows=(y0, y1)` restates a band of rows only, on the whole map:
the rays that leave the band read the rows they reach.  Test infrastructure."""
import numpy as np

from relight_ref import DIRECTIONAL, F, anchor_depth, apply_gain, channel_gains, clamp_depth, inv_r2, shade, unit_direction

I32 = np.int32


def shadow(maxSteps=256, bias=0.0, softness=0.0, strength=1.0):
    """The fields of rtdd_shadow as a dict; the floats are rounded to f32 as the struct holds them."""
    return dict(maxSteps=int(maxSteps), bias=float(F(bias)), softness=float(F(softness)), strength=float(F(strength)))


def directional_step(L):
    """(sx, sy, rise) of a directional light, f32: the unit vector over its larger projected component; None when m == 0."""
    lx, ly, lz = unit_direction(L)
    m = np.fmax(np.abs(lx), np.abs(ly))
    if m == 0:
        return None
    with np.errstate(over="ignore", divide="ignore"):
        return F(lx / m), F(ly / m), F(lz / m)


def shadow_q(depth, L, S, rows=None):
    """q (f32, in [0, 1]) of every pixel of the rows [y0, y1) (default: all), shape (y1 - y0, cols)."""
    depth = np.asarray(depth, F)
    dc = clamp_depth(depth)
    nrows, cols = dc.shape
    y0, y1 = rows if rows is not None else (0, nrows)
    relief = F(L["relief"])
    H = relief * (F(255) - dc)
    ys, xs = (a.ravel().astype(I32) for a in np.mgrid[y0:y1, 0:cols])
    N = xs.size
    q = np.zeros(N, F)
    bias, soft, maxSteps = F(S["bias"]), F(S["softness"]), S["maxSteps"]
    h0 = H[ys, xs] + bias
    with np.errstate(all="ignore"):
        if L["kind"] == DIRECTIONAL:
            step = directional_step(L)
            if step is None:
                return q.reshape(y1 - y0, cols)
            sx, sy, rise = (np.full(N, v, F) for v in step)
            n = np.full(N, maxSteps, I32)
        else:
            Lz = (relief * (F(255) - anchor_depth(depth, L))) + F(L["z"])
            vx, vy, vz = F(L["x"]) - xs.astype(F), F(L["y"]) - ys.astype(F), Lz - H[ys, xs]
            m = np.fmax(np.abs(vx), np.abs(vy))
            sx, sy, rise = vx / m, vy / m, vz / m
            n = np.where(m < 1, 0, np.minimum(maxSteps, np.minimum(m, F(1 << 20)).astype(I32))).astype(I32)
        idx = np.nonzero(n >= 1)[0]
        for k in range(1, maxSteps + 1):
            if idx.size == 0:
                break
            kf = F(k)
            px = xs[idx] + np.rint(kf * sx[idx]).astype(I32)
            py = ys[idx] + np.rint(kf * sy[idx]).astype(I32)
            ok = (px >= 0) & (px < cols) & (py >= 0) & (py < nrows)
            idx, px, py = idx[ok], px[ok], py[ok]                      # the first (px, py) outside the image ends the march
            ray = h0[idx] + (kf * rise[idx])
            occ = H[py, px] - ray
            assert ray.dtype == F and occ.dtype == F
            pos = occ > 0
            qk = np.zeros(idx.size, F)
            qk[pos] = F(1) if soft == 0 else np.fmin(occ[pos] / (kf * soft), F(1))
            q[idx] = np.fmax(q[idx], qk)
            idx = idx[(n[idx] > k) & (q[idx] < 1)]
    assert q.dtype == F
    return q.reshape(y1 - y0, cols)


def visibility(depth, L, S, rows=None):
    """vis = 1 - (strength * q)."""
    return F(1) - (F(S["strength"]) * shadow_q(depth, L, S, rows))


def relight_shadowed(orig, depth, L, S, rows=None):
    """The image (rows=None), or its rows [y0, y1)."""
    depth = np.asarray(depth, F)
    y0, y1 = rows if rows is not None else (0, depth.shape[0])
    s = shade(depth, L)[y0:y1] * visibility(depth, L, S, rows)
    assert s.dtype == F
    return apply_gain(orig[y0:y1], s, L)


def relight_shadowed_literal(orig, depth, L, S, vis_out=None):
    """The header's lines, one pixel at a time, every intermediate an np.float32 scalar.  vis_out: an f32 array that receives vis."""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape

    def dp(x, y):
        d = depth[y, x]
        if d != d:
            return F(0)
        return F(min(max(d, F(0)), F(255)))

    relief, amb = F(L["relief"]), F(L["ambient"])

    def Hh(x, y):
        return F(relief * F(F(255) - dp(x, y)))

    ks = channel_gains(L)
    bias, soft, strength, maxSteps = F(S["bias"]), F(S["softness"]), F(S["strength"]), S["maxSteps"]
    s_all = shade(depth, L)                                   # relight's shade (pinned against its own literal loop by test_relight_cpu.py)
    if L["kind"] == DIRECTIONAL:
        lx, ly, lz = unit_direction(L)
        m = F(max(abs(lx), abs(ly)))
    else:
        dA = dp(L["anchorX"], L["anchorY"]) if L["anchorX"] >= 0 else F(L["anchorDepth"])
        Lz = F(F(relief * F(F(255) - dA)) + F(L["z"]))
    out = np.empty_like(orig)
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                if L["kind"] == DIRECTIONAL:
                    if m == 0:
                        n = 0
                    else:
                        sx, sy, rise, n = F(lx / m), F(ly / m), F(lz / m), maxSteps
                else:
                    vx, vy = F(F(L["x"]) - F(x)), F(F(L["y"]) - F(y))
                    vz = F(Lz - Hh(x, y))
                    mp = F(max(abs(vx), abs(vy)))
                    if mp < 1:
                        n = 0
                    else:
                        sx, sy, rise, n = F(vx / mp), F(vy / mp), F(vz / mp), min(maxSteps, int(mp))
                q = F(0)
                for k in range(1, n + 1):
                    kf = F(k)
                    px, py = x + int(np.rint(F(kf * sx))), y + int(np.rint(F(kf * sy)))
                    if px < 0 or px >= cols or py < 0 or py >= rows:
                        break
                    ray = F(F(Hh(x, y) + bias) + F(kf * rise))
                    occ = F(Hh(px, py) - ray)
                    if not occ > 0:
                        qk = F(0)
                    elif soft == 0:
                        qk = F(1)
                    else:
                        qk = F(min(F(occ / F(kf * soft)), F(1)))
                    q = max(q, qk)
                vis = F(F(1) - F(strength * q))
                if vis_out is not None:
                    vis_out[y, x] = vis
                lit = F(s_all[y, x] * vis)
                for c in range(3):
                    v = F(F(orig[y, x, c]) * F(amb + F(ks[c] * lit)))
                    out[y, x, c] = int(min(v, F(255)))
    return out
