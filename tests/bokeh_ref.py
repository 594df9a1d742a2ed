"""Two independent restatements of the occlusion-aware lens blur (include/rtdd.h rtdd_simulate_bokeh) in numpy and plain Python, written
from the header's text only.

Per pixel q: d' = clamp(d) (a NaN is 0), t = d' - f in f32 (f clamped alike), k = (int)((double)((float)K * |t|) / 255.0), s = -k when t < 0,
else k.  Source q reaches target p iff 4 |q - p|^2 <= ke^2 with ke = min(k_q, k_p) when s_q > s_p, else k_q; out_c = floor(S_c / W) with
W = sum wt[ke], S_c = sum wt[ke] o_c(q) over the sources that reach p, wt[k] = floor(2^30 / N(k)).
  1. bokeh_by_offsets: a loop over the window's (dx, dy), shifted int64 arrays (optionally a band of output rows only).
  2. bokeh_literal: target by target and source by source, Python integers."""
import functools

import numpy as np

from lens_blur_ref import disc_points

KMAX = 127


@functools.lru_cache(maxsize=None)
def _weights():
    return tuple((1 << 30) // disc_points(k) for k in range(KMAX + 1))


def weights():
    """wt[k] = floor(2^30 / N(k)), k = 0 .. 127."""
    return np.array(_weights(), np.int64)


def clamp_depth(d):
    """fminf(fmaxf(d, 0), 255): a NaN gives 0."""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(d), np.float32(0), np.minimum(np.maximum(d, np.float32(0)), np.float32(255))).astype(np.float32)


def signed_coc(depth, f, K):
    """s [rows, cols] (int64) of a depth map for the focus value f (before its clamp) and the window scale K."""
    t = (clamp_depth(depth) - clamp_depth(f)).astype(np.float32)
    kf = (np.float32(K) * np.abs(t)).astype(np.float32).astype(np.float64) / 255.0
    k = np.trunc(kf).astype(np.int64)
    return np.where(t < 0, -k, k)


def bokeh_by_offsets_s(orig, s, band=None):
    """Output rows band = (r0, r1) (default: all) for a given map of signed circles s."""
    rows, cols = s.shape
    r0, r1 = band if band is not None else (0, rows)
    k = np.abs(s)
    wt = weights()
    hmax = int(k.max()) // 2 if k.size else 0                        # no source reaches further, no cap admits more
    # the slab of rows the band's pixels can be reached from, padded by hmax on every side with sources that reach nothing
    pad = hmax
    y0, y1 = max(r0 - pad, 0), min(r1 + pad, rows)
    H, Wd = (r1 - r0) + 2 * pad, cols + 2 * pad
    sq = np.zeros((H, Wd), np.int64); kq = np.zeros((H, Wd), np.int64); inside = np.zeros((H, Wd), bool)
    oq = np.zeros((H, Wd, 3), np.int64)
    a = y0 - (r0 - pad)
    sq[a:a + y1 - y0, pad:pad + cols] = s[y0:y1]; kq[a:a + y1 - y0, pad:pad + cols] = k[y0:y1]; inside[a:a + y1 - y0, pad:pad + cols] = True
    oq[a:a + y1 - y0, pad:pad + cols] = orig[y0:y1]
    sp, kp = s[r0:r1], k[r0:r1]
    W = np.zeros((r1 - r0, cols), np.int64); S = np.zeros((r1 - r0, cols, 3), np.int64)
    for dy in range(-hmax, hmax + 1):
        for dx in range(-hmax, hmax + 1):
            d2 = 4 * (dx * dx + dy * dy)
            if d2 > (2 * hmax + 1) ** 2:
                continue
            ys, xs = slice(pad + dy, pad + dy + r1 - r0), slice(pad + dx, pad + dx + cols)
            ke = np.where(sq[ys, xs] > sp, np.minimum(kq[ys, xs], kp), kq[ys, xs])
            w = np.where(inside[ys, xs] & (d2 <= ke * ke), wt[ke], 0)
            W += w
            S += w[..., None] * oq[ys, xs]
    return (S // W[..., None]).astype(np.uint8), int(S.max()) if S.size else 0


def bokeh_by_offsets(orig, depth, f, K, band=None):
    return bokeh_by_offsets_s(orig, signed_coc(depth, f, K), band)[0]


def bokeh_literal_s(orig, s):
    rows, cols = s.shape
    wt = _weights()
    sl = [[int(v) for v in r] for r in s]
    ol = orig.tolist()
    out = np.empty_like(orig)
    for py in range(rows):
        for px in range(cols):
            sp = sl[py][px]; kp = abs(sp)
            W = 0; S = [0, 0, 0]
            for qy in range(rows):
                for qx in range(cols):
                    sq = sl[qy][qx]; kq = abs(sq)
                    ke = min(kq, kp) if sq > sp else kq
                    if 4 * ((qx - px) ** 2 + (qy - py) ** 2) <= ke * ke:
                        w = wt[ke]
                        W += w
                        o = ol[qy][qx]
                        S[0] += w * o[0]; S[1] += w * o[1]; S[2] += w * o[2]
            out[py, px] = [S[0] // W, S[1] // W, S[2] // W]
    return out


def bokeh_literal(orig, depth, f, K):
    return bokeh_literal_s(orig, signed_coc(depth, f, K))


def two_layer_scene():
    """The scene of the effect's motivation: a red 30 x 30 square at depth 10 on a blue background at depth 200, 70 x 90, K = 40.
    Returns (orig BGR, depth, the square's mask, K)."""
    rows, cols, K = 70, 90, 40
    orig = np.zeros((rows, cols, 3), np.uint8); orig[..., 0] = 255
    depth = np.full((rows, cols), 200.0, np.float32)
    sq = np.zeros((rows, cols), bool); sq[20:50, 30:60] = True
    orig[sq] = (0, 0, 255); depth[sq] = 10.0
    return orig, depth, sq, K
