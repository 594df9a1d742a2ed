"""Two restatements of rtdd_simulate_parallax_layered (include/rtdd.h) for the tests, built on tests/parallax_ref.py's helpers:
`parallax_layers` in vectorised numpy float32 -- a np.minimum.at scatter of both layers on the packed key with the layer bit, the crack
test on every back-won target at once, the holes marched together -- and `parallax_layers_literal`, a loop per pixel over the header's
sentences.  Both return (view, depthOut, coverage).  Neither knows about the kernels' waves, tiles or launches.  Test infrastructure."""
import numpy as np

from parallax_ref import EMPTY, F, a_fields, clamp_depth, intermediates, zero_parallax

LAYER = np.uint64(1 << 31)                      # bit 31 of the key's low word: the source is a plate pixel
INDEX = np.uint64((1 << 31) - 1)
FRONT, BACK, CRACK, MARCHED, LEFT = 0, 1, 2, 3, 4       # the coverage codes


def scatter_layers(depth, plate_depth=None, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1, stats=None):
    """The z-buffer of both layers: per target the packed key bits(d') << 32 | layer << 31 | y * cols + x of its winner (EMPTY: a hole).
    z0 is the FRONT map's.  stats (a dict) receives how many plate sources differ in d' from the front pixel at their own position and
    land inside the image: the atomics a scatter that skips the others issues for the plate."""
    rows, cols = depth.shape
    z = zero_parallax(depth, z0, zx, zy)
    y, x = np.mgrid[0:rows, 0:cols]
    keys = np.full(rows * cols, EMPTY, np.uint64)
    layers = [(depth, np.uint64(0))] + ([(plate_depth, LAYER)] if plate_depth is not None else [])
    for dmap, bit in layers:
        f32, sx, sy = intermediates(dmap, shiftX, shiftY, dolly, z)
        assert all(v.dtype == F for v in f32.values())
        tx, ty = x + sx, y + sy
        ok = (tx >= 0) & (tx < cols) & (ty >= 0) & (ty < rows)
        hi = f32["dc"].view(np.uint32).astype(np.uint64)
        key = (hi << np.uint64(32)) | bit | (y * cols + x).astype(np.uint64)
        np.minimum.at(keys, (ty * cols + tx)[ok], key[ok])
        if bit and stats is not None:
            differs = f32["dc"].view(np.uint32) != clamp_depth(depth).view(np.uint32)
            stats["plate_atomics"] = int((ok & differs).sum())
    return keys.reshape(rows, cols)


def _steps(rows, cols, shiftX, shiftY, dolly):
    """Per pixel: m != 0, and the f32 step (stx, sty) of the hole rule (garbage where m == 0)."""
    ax, ay = a_fields(rows, cols, shiftX, shiftY, dolly)
    AX, AY = np.broadcast_to(ax[None, :], (rows, cols)), np.broadcast_to(ay[:, None], (rows, cols))
    m = np.fmax(np.abs(AX), np.abs(AY))
    with np.errstate(invalid="ignore", divide="ignore"):
        stx, sty = AX / m, AY / m
    assert m.dtype == F and stx.dtype == F and sty.dtype == F
    return m != 0, stx, sty


def cracks(keys, shiftX=0, shiftY=0, dolly=0.0):
    """The crack rule on every target at once: (is a crack, the flat index of its p+)."""
    rows, cols = keys.shape
    filled = keys != EMPTY
    back = filled & ((keys & LAYER) != 0)
    front = filled & ~back
    hi = keys >> np.uint64(32)
    go, stx, sty = _steps(rows, cols, shiftX, shiftY, dolly)
    y, x = np.mgrid[0:rows, 0:cols]
    cand = back & go
    dx = np.where(cand, np.rint(np.where(cand, stx, 0)), 0).astype(np.int64)
    dy = np.where(cand, np.rint(np.where(cand, sty, 0)), 0).astype(np.int64)
    ok = cand
    plus = None
    for sign in (1, -1):
        px, py = x + sign * dx, y + sign * dy
        inside = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
        pxc, pyc = np.clip(px, 0, cols - 1), np.clip(py, 0, rows - 1)
        ok = ok & inside & front[pyc, pxc] & (hi[pyc, pxc] < hi)
        if sign == 1:
            plus = pyc * cols + pxc
    return ok, plus


def resolve_layers(keys, shiftX=0, shiftY=0, dolly=0.0, stats=None):
    """Per target the key of its SOURCE (EMPTY: none, the hole keeps the original) and the coverage code."""
    rows, cols = keys.shape
    filled = keys != EMPTY
    crack, plus = cracks(keys, shiftX, shiftY, dolly)
    skey = np.where(crack, keys.reshape(-1)[plus], keys)           # a crack's source is its p+'s (front-won: never a crack itself)
    cov = np.where(crack, CRACK, np.where((keys & LAYER) != 0, BACK, FRONT)).astype(np.uint8)
    cov[~filled] = LEFT
    hy, hx = np.nonzero(~filled)
    go, stx, sty = _steps(rows, cols, shiftX, shiftY, dolly)
    go, stx, sty = go[hy, hx], stx[hy, hx], sty[hy, hx]
    resolved = ~go
    for sign in (1, -1):
        act = np.flatnonzero(~resolved)
        k = 0
        while act.size:
            k += 1
            kf = F(k)
            px = hx[act] + sign * np.rint(kf * stx[act]).astype(np.int64)
            py = hy[act] + sign * np.rint(kf * sty[act]).astype(np.int64)
            inside = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
            act, px, py = act[inside], px[inside], py[inside]
            hit = filled[py, px]
            done = act[hit]
            skey[hy[done], hx[done]] = skey[py[hit], px[hit]]
            cov[hy[done], hx[done]] = MARCHED
            resolved[done] = True
            act = act[~hit]
    if stats is not None:
        n = max(rows * cols, 1)
        stats["holes"] = hy.size / n
        stats["left"] = int((cov == LEFT).sum()) / n
        stats["cracks"] = int(crack.sum()) / n
    return skey, cov


def parallax_layers(orig, depth, plate=None, plate_depth=None, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1, stats=None):
    """rtdd_simulate_parallax_layered restated in numpy: orig, plate rows x cols x 3 u8 (BGR), depth, plate_depth rows x cols f32; the
    plate both or neither None.  Returns (view u8 x 3, depthOut f32, coverage u8)."""
    assert (plate is None) == (plate_depth is None)
    rows, cols = depth.shape
    keys = scatter_layers(depth, plate_depth, shiftX, shiftY, dolly, z0, zx, zy, stats)
    skey, cov = resolve_layers(keys, shiftX, shiftY, dolly, stats)
    own = (np.arange(rows * cols).reshape(rows, cols)).astype(np.uint64)
    none = skey == EMPTY
    idx = np.where(none, own, skey & INDEX).astype(np.int64).reshape(-1)
    from_plate = (~none & ((skey & LAYER) != 0)).reshape(-1)
    colours = orig.reshape(rows * cols, 3)[idx]
    if plate is not None:
        colours = np.where(from_plate[:, None], plate.reshape(rows * cols, 3)[idx], colours)
    else:
        assert not from_plate.any()
    dout = np.where(none, clamp_depth(depth).view(np.uint32), (skey >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F)
    assert dout.dtype == F
    return colours.reshape(rows, cols, 3), dout, cov


def parallax_layers_literal(orig, depth, plate=None, plate_depth=None, shiftX=0, shiftY=0, dolly=0.0, z0=0.0, zx=-1, zy=-1):
    """The header's sentences, one pixel at a time (small images only)."""
    assert (plate is None) == (plate_depth is None)
    rows, cols = depth.shape

    def clamp(v):
        v = F(v)
        return F(0) if v != v else F(min(max(v, F(0)), F(255))) + F(0)

    def a(x, y):
        return F(F(shiftX) - F(F(dolly) * F(F(x) - cx))), F(F(shiftY) - F(F(dolly) * F(F(y) - cy)))

    def rint(v):
        return int(np.rint(F(v)))

    def inside(p):
        return 0 <= p[0] < cols and 0 <= p[1] < rows

    z = F(z0) if zx < 0 else clamp(depth[zy, zx])
    cx, cy = F(F(cols - 1) * F(0.5)), F(F(rows - 1) * F(0.5))
    win = {}                                                        # target -> (d', layer, y * cols + x) of the winner
    for layer, dmap in ((0, depth), (1, plate_depth)):
        if dmap is None:
            continue
        for y in range(rows):
            for x in range(cols):
                dc = clamp(dmap[y, x])
                ax, ay = a(x, y)
                dz = F(dc - z)
                t = (x + rint(F(F(ax * dz) / F(255))), y + rint(F(F(ay * dz) / F(255))))
                if not inside(t):
                    continue
                cand = (dc, layer, y * cols + x)
                if t not in win or (float(cand[0]), cand[1], cand[2]) < (float(win[t][0]), win[t][1], win[t][2]):
                    win[t] = cand

    def step(x, y):
        ax, ay = a(x, y)
        m = F(max(abs(ax), abs(ay)))
        return (None, None) if m == 0 else (F(ax / m), F(ay / m))

    def source(t):
        """(the winner whose colour and depth the FILLED target t shows, is t a crack)"""
        w = win[t]
        if w[1] == 0:
            return w, False
        stx, sty = step(*t)
        if stx is None:
            return w, False
        dx, dy = rint(stx), rint(sty)
        pp, pm = (t[0] + dx, t[1] + dy), (t[0] - dx, t[1] - dy)
        for p in (pp, pm):
            if not (inside(p) and p in win and win[p][1] == 0 and float(win[p][0]) < float(w[0])):
                return w, False
        return win[pp], True

    def march(x, y, stx, sty, sign):
        k = 0
        while True:
            k += 1
            p = (x + sign * rint(F(F(k) * stx)), y + sign * rint(F(F(k) * sty)))
            if not inside(p):
                return None
            if p in win:
                return source(p)[0]

    images = (orig.reshape(rows * cols, 3), plate.reshape(rows * cols, 3) if plate is not None else None)
    view, dout, cov = np.empty_like(orig), np.empty((rows, cols), F), np.empty((rows, cols), np.uint8)
    for y in range(rows):
        for x in range(cols):
            if (x, y) in win:
                w, crack = source((x, y))
                code = CRACK if crack else (BACK if w[1] else FRONT)
            else:
                w, code = None, LEFT
                stx, sty = step(x, y)
                if stx is not None:
                    w = march(x, y, stx, sty, 1)
                    if w is None:
                        w = march(x, y, stx, sty, -1)
                    if w is not None:
                        code = MARCHED
            cov[y, x] = code
            if w is None:
                view[y, x], dout[y, x] = orig[y, x], clamp(depth[y, x])
            else:
                view[y, x], dout[y, x] = images[w[1]][w[2]], w[0]
    return view, dout, cov
