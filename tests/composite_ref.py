"""Two restatements of rtdd_composite_layer (include/rtdd.h) for the tests: `composite` in vectorised numpy (64-bit integers, float32 for
steps 3 - 4) and `composite_literal`, a per-pixel loop over the header's lines in Python integers with numpy.float32 scalars.  Neither
knows about the kernel: there is no footprint, every pixel of the image goes through step 1.  Both return (artistic, depthOut); the
depth of a pixel the layer does not win is the input's, bit for bit.  Test infrastructure."""
import numpy as np

F = np.float32
I64 = np.int64
NEAREST, BILINEAR = 0, 1
E = 255 * 255 * 256


def layer(rows, cols, x=0, y=0, scale=256, filter=NEAREST, opacity=255, x0=0, y0=0, x1=0, y1=0, depth0=0.0, depth1=0.0, feather=0.0):
    """The fields of rtdd_layer as a dict; the floats are rounded to f32 as the struct holds them."""
    return dict(rows=int(rows), cols=int(cols), x=int(x), y=int(y), scale=int(scale), filter=int(filter), opacity=int(opacity),
                x0=int(x0), y0=int(y0), x1=int(x1), y1=int(y1), depth0=float(F(depth0)), depth1=float(F(depth1)), feather=float(F(feather)))


def random_sprite(rows, cols, seed, alpha="random"):
    """A u8 x 4 sprite (B, G, R, A).  alpha: 0, 255, "ramp" or "random" (30 % transparent); a transparent texel carries colour 255, so any
    bleed shows."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    if alpha == "ramp":
        s[..., 3] = np.linspace(0, 255, cols).astype(np.uint8)[None, :]
    elif alpha == "random":
        s[..., 3] = np.where(rng.random((rows, cols)) < 0.3, 0, s[..., 3])
    else:
        s[..., 3] = alpha
    s[s[..., 3] == 0, :3] = 255
    return s


def _coord(p, origin, scale):
    """U + 128 of step 1 for the pixel indices p (int64): floor division."""
    return ((2 * (p - origin) + 1) * 32768) // scale


def layer_depth(L, rows, cols):
    """z of step 3 for every pixel, f32 (rows, cols)."""
    ax, ay = L["x1"] - L["x0"], L["y1"] - L["y0"]
    dd = ax * ax + ay * ay
    if dd == 0:
        return np.full((rows, cols), F(L["depth0"]), F)
    px, py = np.arange(cols, dtype=I64), np.arange(rows, dtype=I64)
    n = np.clip(((px - L["x0"]) * ax)[None, :] + ((py - L["y0"]) * ay)[:, None], 0, dd)
    assert int(n.max()) < 2 ** 31
    frac = n.astype(F) / F(dd)
    z = F(L["depth0"]) + ((F(L["depth1"]) - F(L["depth0"])) * frac)
    assert z.dtype == F
    return z


def visibility(depth, z, feather):
    """v of step 4, int64 in 0 .. 256."""
    with np.errstate(all="ignore"):
        dc = np.fmin(np.fmax(np.asarray(depth, F), F(0)), F(255))          # fmax / fmin drop a NaN: it becomes 0
        diff = dc - z
        assert diff.dtype == F
        if feather == 0:
            return np.where(diff >= 0, 256, 0).astype(I64)
        t = (diff / F(feather)) + F(0.5)
        v = np.fmin(np.fmax(t, F(0)), F(1)) * F(256)
        assert v.dtype == F
        return v.astype(I64)


def sample(sprite, L, rows, cols):
    """Steps 1 - 2 for every pixel of a rows x cols image: (covered (rows, cols) bool, c (rows, cols, 3) int64, a (rows, cols) int64);
    c and a are 0 where the pixel is not covered."""
    sr, sc = L["rows"], L["cols"]
    assert sprite.shape == (sr, sc, 4) and sprite.dtype == np.uint8
    qx = _coord(np.arange(cols, dtype=I64), L["x"], L["scale"])
    qy = _coord(np.arange(rows, dtype=I64), L["y"], L["scale"])
    covered = ((qy >= 0) & (qy < 256 * sr))[:, None] & ((qx >= 0) & (qx < 256 * sc))[None, :]
    S = sprite.astype(I64)
    if L["filter"] == NEAREST:
        t = S[np.clip(qy >> 8, 0, sr - 1)[:, None], np.clip(qx >> 8, 0, sc - 1)[None, :]]
        c, a = t[..., :3], t[..., 3]
    else:
        U, V = qx - 128, qy - 128
        iu, iv = U >> 8, V >> 8                                              # (>> floors a negative int64)
        fu, fv = U - 256 * iu, V - 256 * iv
        A = np.zeros((rows, cols), I64); Cc = np.zeros((rows, cols, 3), I64)
        for dy, wy in ((0, 256 - fv), (1, fv)):
            for dx, wx in ((0, 256 - fu), (1, fu)):
                t = S[np.clip(iv + dy, 0, sr - 1)[:, None], np.clip(iu + dx, 0, sc - 1)[None, :]]
                w = wy[:, None] * wx[None, :]
                A += w * t[..., 3]
                Cc += (w * t[..., 3])[..., None] * t[..., :3]
        assert int(A.max()) < 2 ** 24 and int(Cc.max()) < 2 ** 32
        a = (A + 32768) >> 16
        c = np.where(A[..., None] > 0, (Cc + (A >> 1)[..., None]) // np.maximum(A, 1)[..., None], 0)
    return covered, np.where(covered[..., None], c, 0), np.where(covered, a, 0)


def composite(orig, depth, sprite, L):
    """(artistic u8 (rows, cols, 3), depthOut f32 (rows, cols)) of the header's rule."""
    depth = np.ascontiguousarray(depth, F)
    rows, cols = depth.shape
    covered, c, a = sample(sprite, L, rows, cols)
    z = layer_depth(L, rows, cols)
    v = visibility(depth, z, L["feather"])
    e = np.where(covered, a * L["opacity"] * v, 0)
    assert int(e.max(initial=0)) <= E
    num = c * e[..., None] + orig.astype(I64) * (E - e)[..., None] + E // 2
    assert int(num.max(initial=0)) < 2 ** 32
    art = (num // E).astype(np.uint8)
    wins = 2 * e >= E
    dout = depth.copy()
    dout[wins] = z[wins]
    return art, dout


def composite_literal(orig, depth, sprite, L):
    """The header's lines, one pixel at a time: Python integers, and np.float32 scalars for steps 3 - 4."""
    depth = np.ascontiguousarray(depth, F)
    rows, cols = depth.shape
    sr, sc, scale = L["rows"], L["cols"], L["scale"]
    art, dout = orig.copy(), depth.copy()                                    # an uncovered pixel: the original, the depth's bits
    S = sprite.tolist()
    ax, ay = L["x1"] - L["x0"], L["y1"] - L["y0"]
    dd = ax * ax + ay * ay
    d0, d1, feather = F(L["depth0"]), F(L["depth1"]), F(L["feather"])

    def clamp(i, n):
        return min(max(i, 0), n - 1)

    with np.errstate(all="ignore"):
        for py in range(rows):
            V = ((2 * (py - L["y"]) + 1) * 32768) // scale - 128
            if not 0 <= V + 128 < 256 * sr:
                continue
            for px in range(cols):
                U = ((2 * (px - L["x"]) + 1) * 32768) // scale - 128
                if not 0 <= U + 128 < 256 * sc:
                    continue
                if L["filter"] == NEAREST:
                    cb, cg, cr, a = S[(V + 128) // 256][(U + 128) // 256]
                    c = (cb, cg, cr)
                else:
                    iu, iv = U // 256, V // 256
                    fu, fv = U - 256 * iu, V - 256 * iv
                    A, C = 0, [0, 0, 0]
                    for ty, wy in ((iv, 256 - fv), (iv + 1, fv)):
                        for tx, wx in ((iu, 256 - fu), (iu + 1, fu)):
                            t = S[clamp(ty, sr)][clamp(tx, sc)]
                            A += wy * wx * t[3]
                            for k in range(3):
                                C[k] += wy * wx * t[3] * t[k]
                    a = (A + 32768) >> 16
                    c = tuple((C[k] + (A >> 1)) // A if A else 0 for k in range(3))
                if dd:
                    n = min(max((px - L["x0"]) * ax + (py - L["y0"]) * ay, 0), dd)
                    z = F(d0 + F(F(d1 - d0) * F(F(n) / F(dd))))
                else:
                    z = d0
                d = depth[py, px]
                dc = F(0) if d != d else F(min(max(d, F(0)), F(255)))
                diff = F(dc - z)
                if feather == 0:
                    v = 256 if diff >= 0 else 0
                else:
                    t = F(F(diff / feather) + F(0.5))
                    v = int(F(F(min(max(t, F(0)), F(1))) * F(256)))
                e = a * L["opacity"] * v
                for k in range(3):
                    art[py, px, k] = (c[k] * e + int(orig[py, px, k]) * (E - e) + E // 2) // E
                if 2 * e >= E:
                    dout[py, px] = z
    return art, dout


def same_bits(a, b):
    """Two f32 arrays are equal bit for bit, NaN payloads included."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
