"""Two restatements of rtdd_simulate_parallax (include/rtdd.h) for the tests: `parallax` in vectorised numpy float32 -- a
np.minimum.at scatter on the packed key, the holes marched together step by step -- and `parallax_literal`, a loop per pixel over
the rules as the header states them.  Neither knows about the kernels' waves, tiles or launches.  Test infrastructure."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def clamp_depth(d):
    """d' = fminf(fmaxf(d, 0), 255) in f32: a NaN depth is 0, -0 counts as +0."""
    return np.fmin(np.fmax(np.asarray(d, F), F(0)), F(255)) + F(0)


def zero_parallax(depth, z0=0.0, zx=-1, zy=-1):
    return F(z0) if zx < 0 else clamp_depth(depth[zy, zx])


def a_fields(rows, cols, shiftX, shiftY, dolly):
    """ax per column and ay per row: (float)shift - (dolly * ((float)x - c)), c = (float)(n - 1) * 0.5f."""
    cx, cy = F(cols - 1) * F(0.5), F(rows - 1) * F(0.5)
    ax = F(shiftX) - (F(dolly) * (np.arange(cols).astype(F) - cx))
    ay = F(shiftY) - (F(dolly) * (np.arange(rows).astype(F) - cy))
    assert ax.dtype == F and ay.dtype == F and cx.dtype == F and cy.dtype == F
    return ax, ay


def intermediates(depth, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1):
    """Every f32 intermediate of the source rule, by name, and the integer shifts (sx, sy)."""
    rows, cols = depth.shape
    dc = clamp_depth(depth)
    z = zero_parallax(depth, z0, zx, zy)
    ax, ay = a_fields(rows, cols, shiftX, shiftY, dolly)
    dz = dc - z
    px, py = ax[None, :] * dz, ay[:, None] * dz
    qx, qy = px / F(255), py / F(255)
    f32 = dict(dc=dc, z=z, ax=ax, ay=ay, dz=dz, px=px, py=py, qx=qx, qy=qy)
    return f32, np.rint(qx).astype(np.int64), np.rint(qy).astype(np.int64)


def scatter(depth, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1):
    """The z-buffer: per target the packed key bits(d') << 32 | y * cols + x of its winner (EMPTY: a hole), rows x cols u64; and per
    target how many sources share the winner's d' (>= 2: the smallest-index rule decided)."""
    rows, cols = depth.shape
    f32, sx, sy = intermediates(depth, shiftX, shiftY, dolly, z0, zx, zy)
    assert all(v.dtype == F for v in f32.values())
    y, x = np.mgrid[0:rows, 0:cols]
    tx, ty = x + sx, y + sy
    ok = (tx >= 0) & (tx < cols) & (ty >= 0) & (ty < rows)
    hi = f32["dc"].view(np.uint32).astype(np.uint64)
    key = (hi << np.uint64(32)) | (y * cols + x).astype(np.uint64)
    keys = np.full(rows * cols, EMPTY, np.uint64)
    t = (ty * cols + tx)[ok]
    np.minimum.at(keys, t, key[ok])
    same = np.zeros(rows * cols, np.int64)
    np.add.at(same, t, (hi[ok] == (keys[t] >> np.uint64(32))).astype(np.int64))
    return keys.reshape(rows, cols), same.reshape(rows, cols)


def resolve(keys, shiftX=0, shiftY=0, dolly=0.0, stats=None):
    """Per target the index y * cols + x of the source whose colour the view takes.  stats (a dict) receives the share of holes and
    the mean number of targets a hole's marches look at."""
    rows, cols = keys.shape
    filled = keys != EMPTY
    src = np.where(filled, keys & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    hy, hx = np.nonzero(~filled)
    out = src.copy()
    out[hy, hx] = hy * cols + hx                                   # m == 0, or both marches end: original[t]
    ax, ay = a_fields(rows, cols, shiftX, shiftY, dolly)
    hax, hay = ax[hx], ay[hy]
    m = np.fmax(np.abs(hax), np.abs(hay))
    go = m != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        stx, sty = hax / m, hay / m
    assert stx.dtype == F and sty.dtype == F and m.dtype == F
    looked = 0
    resolved = ~go                                                 # per hole: nothing (more) to march for
    for sign in (1, -1):
        act = np.flatnonzero(~resolved)                            # the holes still marching in this direction
        k = 0
        while act.size:
            k += 1
            kf = F(k)
            px = hx[act] + sign * np.rint(kf * stx[act]).astype(np.int64)
            py = hy[act] + sign * np.rint(kf * sty[act]).astype(np.int64)
            inside = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
            act, px, py = act[inside], px[inside], py[inside]
            looked += act.size
            hit = filled[py, px]
            done = act[hit]
            out[hy[done], hx[done]] = src[py[hit], px[hit]]
            resolved[done] = True
            act = act[~hit]
    if stats is not None:
        stats["holes"] = hy.size / max(rows * cols, 1)
        stats["march"] = looked / max(hy.size, 1)
    return out


def parallax(orig, depth, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1, stats=None):
    """rtdd_simulate_parallax restated in numpy: orig rows x cols x 3 u8 (BGR), depth rows x cols f32."""
    rows, cols = depth.shape
    keys, _ = scatter(depth, shiftX, shiftY, dolly, z0, zx, zy)
    src = resolve(keys, shiftX, shiftY, dolly, stats)
    return orig.reshape(rows * cols, 3)[src.reshape(-1)].reshape(rows, cols, 3)


def parallax_literal(orig, depth, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1):
    """The header's rules, one pixel at a time (small images only)."""
    rows, cols = depth.shape

    def clamp(v):
        v = F(v)
        return F(0) if v != v else F(min(max(v, F(0)), F(255))) + F(0)

    def a(x, y):
        return F(F(shiftX) - F(F(dolly) * F(F(x) - cx))), F(F(shiftY) - F(F(dolly) * F(F(y) - cy)))

    def rint(v):
        return int(np.rint(F(v)))

    z = F(z0) if zx < 0 else clamp(depth[zy, zx])
    cx, cy = F(F(cols - 1) * F(0.5)), F(F(rows - 1) * F(0.5))
    win = {}                                                        # target -> (d', y * cols + x) of the winner
    for y in range(rows):
        for x in range(cols):
            dc = clamp(depth[y, x])
            ax, ay = a(x, y)
            dz = F(dc - z)
            sx, sy = rint(F(F(ax * dz) / F(255))), rint(F(F(ay * dz) / F(255)))
            t = (x + sx, y + sy)
            if not (0 <= t[0] < cols and 0 <= t[1] < rows):
                continue
            cand = (float(dc), y * cols + x)
            if t not in win or cand < win[t]:
                win[t] = cand

    def march(x, y, stx, sty, sign):
        k = 0
        while True:
            k += 1
            p = (x + sign * rint(F(F(k) * stx)), y + sign * rint(F(F(k) * sty)))
            if not (0 <= p[0] < cols and 0 <= p[1] < rows):
                return None
            if p in win:
                return win[p][1]

    flat = orig.reshape(rows * cols, 3)
    out = np.empty_like(orig)
    for y in range(rows):
        for x in range(cols):
            if (x, y) in win:
                out[y, x] = flat[win[(x, y)][1]]
                continue
            ax, ay = a(x, y)
            m = F(max(abs(ax), abs(ay)))
            s = None
            if m != 0:
                stx, sty = F(ax / m), F(ay / m)
                s = march(x, y, stx, sty, 1)
                if s is None:
                    s = march(x, y, stx, sty, -1)
            out[y, x] = flat[s] if s is not None else orig[y, x]
    return out
