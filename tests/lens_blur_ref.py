"""Three independent restatements of the round-aperture lens blur (include/rtdd.h rtdd_simulate_lens_blur, RTDD_APERTURE_DISC) in numpy.

Per pixel (x, y): k = (int)((double)((float)K * |d - f|) / 255.0) clamped to [0, 255] (0 for a NaN), the window is the image's pixels (px, py)
with 4 ((px - x)^2 + (py - y)^2) <= k^2, out = (uchar)(sum / count) per channel in f32.
  1. lens_blur_literal: the mask over the clipped bounding box, pixel by pixel, sums in f32.
  2. lens_blur_by_row_prefixes: one cumsum along x, a loop over dy, isqrt spans, in int64 (optionally a band of output rows only).
  3. lens_blur_constant_k: scipy.ndimage correlation of the image and of an all-ones image with the disc mask -- a constant k only."""
import numpy as np

from refocus_ref import focus_distance, kernel_size


def disc_diameter(K, dist):
    """k of the header: refocus_ref._half_width's arithmetic (int * float -> float, / double, truncation) with the clamp to [0, 255]."""
    with np.errstate(invalid="ignore", over="ignore"):
        kf = (np.float32(K) * dist.astype(np.float32)).astype(np.float64) / 255.0
        k = np.where(np.isnan(kf) | (kf <= 0), 0.0, np.where(kf >= 255, 255.0, np.trunc(kf)))
    return k.astype(np.int64)


def disc_points(k):
    """How many (dx, dy) satisfy 4 (dx^2 + dy^2) <= k^2: counted point by point."""
    h = k // 2
    return sum(1 for dy in range(-h, h + 1) for dx in range(-h, h + 1) if 4 * (dx * dx + dy * dy) <= k * k)


def _store(s, cnt):
    q = s.astype(np.float32) / cnt.astype(np.float32)                  # (uchar)(sum / count) in f32
    return np.clip(np.trunc(q), 0, 255).astype(np.uint8)


def lens_blur_literal_k(orig, k):
    rows, cols = k.shape
    out = np.empty_like(orig)
    for y in range(rows):
        for x in range(cols):
            kk = int(k[y, x]); h = kk // 2
            y0, y1, x0, x1 = max(y - h, 0), min(y + h, rows - 1), max(x - h, 0), min(x + h, cols - 1)
            py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            m = 4 * ((px - x) ** 2 + (py - y) ** 2) <= kk * kk
            win = orig[y0:y1 + 1, x0:x1 + 1]
            cnt = np.float32(m.sum())
            for c in range(3):
                s = win[..., c][m].astype(np.float32).sum(dtype=np.float32)     # f32 accumulation: exact below 2^24 in any order
                out[y, x, c] = np.uint8(min(max(int(np.float32(s / cnt)), 0), 255))
    return out


def lens_blur_literal(orig, depth, f, aperture=0.025):
    rows, cols = depth.shape
    return lens_blur_literal_k(orig, disc_diameter(kernel_size(rows, cols, aperture), focus_distance(depth, f)))


def _isqrt(n):
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r -= (r * r > n)
    r += ((r + 1) * (r + 1) <= n)
    return r


def lens_blur_by_row_prefixes_k(orig, k, band=None):
    """Output rows band = (r0, r1) (default: all) of the disc blur with per-pixel diameters k [rows, cols]."""
    rows, cols = k.shape
    r0, r1 = band if band is not None else (0, rows)
    kb = k[r0:r1]
    hmax = int(kb.max()) // 2 if kb.size else 0
    s0, s1 = max(r0 - hmax, 0), min(r1 + hmax, rows)                   # the slab of image rows the band's discs reach
    P = np.zeros((s1 - s0, cols + 1, 3), np.int64)
    np.cumsum(orig[s0:s1].astype(np.int64), axis=1, out=P[:, 1:])
    yy, xx = np.mgrid[r0:r1, 0:cols]
    yy = yy.ravel(); xx = xx.ravel(); kk = kb.ravel()
    hh = kk // 2; q4 = (kk * kk) // 4
    s = np.zeros((kk.size, 3), np.int64); cnt = np.zeros(kk.size, np.int64)
    for dy in range(-hmax, hmax + 1):
        i = np.nonzero((hh >= abs(dy)) & (yy + dy >= 0) & (yy + dy < rows))[0]
        if i.size == 0:
            continue
        w = _isqrt(q4[i] - dy * dy)
        xa = np.maximum(xx[i] - w, 0); xb = np.minimum(xx[i] + w + 1, cols)
        r = yy[i] + dy - s0
        s[i] += P[r, xb] - P[r, xa]
        cnt[i] += xb - xa
    return _store(s, cnt[:, None]).reshape(r1 - r0, cols, 3)


def lens_blur_by_row_prefixes(orig, depth, f, aperture=0.025, band=None):
    rows, cols = depth.shape
    return lens_blur_by_row_prefixes_k(orig, disc_diameter(kernel_size(rows, cols, aperture), focus_distance(depth, f)), band)


def lens_blur_constant_k(orig, k):
    """Every pixel with the same diameter k: two correlations with the disc mask, zeros beyond the border."""
    from scipy import ndimage
    h = k // 2
    dy, dx = np.mgrid[-h:h + 1, -h:h + 1]
    mask = (4 * (dx * dx + dy * dy) <= k * k).astype(np.float64)
    cnt = ndimage.correlate(np.ones(orig.shape[:2]), mask, mode="constant", cval=0.0)
    out = np.empty_like(orig)
    for c in range(3):
        s = ndimage.correlate(orig[..., c].astype(np.float64), mask, mode="constant", cval=0.0)       # exact: integers below 2^53
        out[..., c] = _store(np.rint(s), np.rint(cnt))
    return out
