"""Two restatements of rtdd_simulate_stereo (include/rtdd.h) for the tests: `stereo` in vectorised numpy float32, and
`stereo_literal`, a per-pixel loop over the rules as the header states them.  Neither knows about the kernel's segments.
Test infrastructure."""
import numpy as np

VIEW, ANAGLYPH = 0, 1


def clamp_depth(d):
    """d' = fminf(fmaxf(d, 0), 255) in f32: a NaN depth is 0."""
    return np.fmin(np.fmax(np.asarray(d, np.float32), np.float32(0)), np.float32(255))


def shifts(depth, D, z0):
    """s = (int)rintf(((float)D * (d' - z0)) / 255.0f), each operation rounded in f32."""
    q = (np.float32(D) * (clamp_depth(depth) - np.float32(z0))) / np.float32(255)
    assert q.dtype == np.float32
    return np.rint(q).astype(np.int64)


def zero_parallax(depth, z0=0.0, zx=-1, zy=-1):
    return np.float32(z0) if zx < 0 else clamp_depth(depth[zy, zx])


def compose(orig, view, D, mode):
    if mode == VIEW:
        return view
    out = view.copy()
    if D >= 0:
        out[..., 2] = orig[..., 2]                  # (view.b, view.g, orig.r)
    else:
        out[..., :2] = orig[..., :2]                # (orig.b, orig.g, view.r)
    return out


def stereo_sources(depth, D, z0):
    """Per target: the source whose colour the view takes (-1: no filled target in the row: original[t]), and the filled mask."""
    rows, cols = depth.shape
    s = shifts(depth, D, z0)
    sg = -1 if D < 0 else 1
    x = np.broadcast_to(np.arange(cols), (rows, cols))
    t = x + s
    ok = (t >= 0) & (t < cols)
    none = 1 << 20
    key = np.full(rows * cols, none, np.int64)     # the nearest source wins: the least sign(D) * s + 256 per target (no ties)
    r = np.broadcast_to(np.arange(rows)[:, None], (rows, cols))
    np.minimum.at(key, r[ok] * cols + t[ok], sg * s[ok] + 256)
    key = key.reshape(rows, cols)
    filled = key < none
    tt = np.broadcast_to(np.arange(cols), (rows, cols))
    src_f = np.where(filled, tt - sg * (key - 256), -1)
    left = np.maximum.accumulate(np.where(filled, tt, -1), axis=1)               # nearest filled at or left of each target
    right = np.minimum.accumulate(np.where(filled, tt, cols)[:, ::-1], axis=1)[:, ::-1]
    right = np.where(right >= cols, -1, right)
    pick = np.where(right >= 0, right, left) if D > 0 else np.where(left >= 0, left, right)
    src = np.where(pick >= 0, np.take_along_axis(src_f, np.maximum(pick, 0), axis=1), -1)
    return src, filled


def stereo(orig, depth, D, z0=0.0, zx=-1, zy=-1, mode=VIEW, chunk=256):
    """rtdd_simulate_stereo restated in numpy: orig rows x cols x 3 u8 (BGR), depth rows x cols f32 (in row chunks)."""
    rows, cols = depth.shape
    z = zero_parallax(depth, z0, zx, zy)
    out = np.empty_like(orig)
    for r0 in range(0, rows, chunk):
        o, d = orig[r0:r0 + chunk], depth[r0:r0 + chunk]
        src, _ = stereo_sources(d, D, z)
        x = np.where(src >= 0, src, np.arange(cols)[None, :])
        view = np.take_along_axis(o, x[..., None].repeat(3, 2), axis=1)
        out[r0:r0 + chunk] = compose(o, view, D, mode)
    return out


def stereo_literal(orig, depth, D, z0=0.0, zx=-1, zy=-1, mode=VIEW):
    """The header's rules, one pixel at a time (small images only)."""
    rows, cols = depth.shape
    f32 = np.float32

    def clamp(v):
        v = f32(v)
        return f32(0) if v != v else f32(min(max(v, f32(0)), f32(255)))

    z = f32(z0) if zx < 0 else clamp(depth[zy, zx])
    sg = -1 if D < 0 else 1
    out = np.empty_like(orig)
    for y in range(rows):
        win = [None] * cols                         # (s * sign(D), x) of the winner
        for x in range(cols):
            s = int(np.rint(f32(f32(f32(D) * f32(clamp(depth[y, x]) - z)) / f32(255))))
            t = x + s
            if 0 <= t < cols and (win[t] is None or s * sg < win[t][0]):
                win[t] = (s * sg, x)
        view = np.empty((cols, 3), np.uint8)
        for t in range(cols):
            if win[t] is not None:
                view[t] = orig[y, win[t][1]]
                continue
            rights = [u for u in range(t + 1, cols) if win[u] is not None]
            lefts = [u for u in range(t - 1, -1, -1) if win[u] is not None]
            first, second = (rights, lefts) if D > 0 else (lefts, rights)
            near = first or second
            view[t] = orig[y, win[near[0]][1]] if near else orig[y, t]
        out[y] = compose(orig[y], view, D, mode)
    return out


def hole_runs(filled_row):
    """(start, length, whole_row) of every run of unfilled targets in one row."""
    runs, t, n = [], 0, len(filled_row)
    while t < n:
        if filled_row[t]:
            t += 1
            continue
        u = t
        while u < n and not filled_row[u]:
            u += 1
        runs.append((t, u - t, t == 0 and u == n))
        t = u
    return runs
