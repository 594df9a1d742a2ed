"""Independent restatements of the aimed depth effects (include/rtdd.h rtdd_simulate_refocus, rtdd_simulate_haze_ex) for the tests.

Refocus: the defocus window of src/GPUDepthEffect.cu:42-70 with K = (int)(aperture * sqrtf(rows^2 + cols^2)) and |d - f| in place of
the depth -- an O(N) 64-bit summed-area table in numpy, and a literal per-pixel gather for small images.  Haze: the blend evaluated
exactly with fractions.Fraction, rounded to f32 once per IEEE operation, with t from the oracle's deterministic exp."""
from fractions import Fraction

import numpy as np


def kernel_size(rows, cols, aperture):
    """(int)(aperture * sqrtf(rows*rows + cols*cols)): a double times an f32 square root, truncated."""
    return int(aperture * float(np.sqrt(np.float32(rows * rows + cols * cols))))


def largest_aperture(rows, cols):
    """An aperture that gives K = 255 exactly, the largest K the library accepts."""
    a = 255.5 / float(np.sqrt(np.float32(rows * rows + cols * cols)))
    assert kernel_size(rows, cols, a) == 255
    return a


def focus_distance(depth, f):
    return np.abs(depth - np.float32(f)).astype(np.float32)


def _half_width(K, dist):
    kf = (np.float32(K) * dist).astype(np.float64) / 255.0           # int * float -> float, / double
    k = np.trunc(np.clip(kf, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    return np.where(k >= 0, k // 2, -((-k) // 2))                    # C integer division truncates toward zero


def _quotient(s, cnt, o):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = s.astype(np.float32) / cnt.astype(np.float32)
    return np.where(cnt > 0, np.clip(np.trunc(q), 0, 255), o).astype(np.uint8)


def refocus_by_summed_area_table(orig, depth, f, aperture=0.025):
    rows, cols = depth.shape
    h = _half_width(kernel_size(rows, cols, aperture), focus_distance(depth, f))
    y = np.arange(rows)[:, None]; x = np.arange(cols)[None, :]
    y0 = np.clip(y - h, 0, rows); y1 = np.clip(y + h, 0, rows); x0 = np.clip(x - h, 0, cols); x1 = np.clip(x + h, 0, cols)
    cnt = np.maximum(y1 - y0, 0) * np.maximum(x1 - x0, 0)
    out = np.empty_like(orig)
    for c in range(3):
        S = np.zeros((rows + 1, cols + 1), np.int64)
        np.cumsum(np.cumsum(orig[..., c].astype(np.int64), 0), 1, out=S[1:, 1:])
        out[..., c] = _quotient(S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0], cnt, orig[..., c])
    return out


def refocus_literal(orig, depth, f, aperture=0.025):
    """The reference's gather loop (src/GPUDepthEffect.cu:47-70) pixel by pixel, with |d - f| as the depth."""
    rows, cols = depth.shape
    h = _half_width(kernel_size(rows, cols, aperture), focus_distance(depth, f))
    out = np.empty_like(orig)
    for yy in range(rows):
        for xx in range(cols):
            k2 = int(h[yy, xx])
            ys = [py for py in range(yy - k2, yy + k2) if 0 <= py < rows]
            xs = [px for px in range(xx - k2, xx + k2) if 0 <= px < cols]
            if not ys or not xs:
                out[yy, xx] = orig[yy, xx]
                continue
            win = orig[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].astype(np.int64)
            cnt = np.float32(len(ys) * len(xs))
            for c in range(3):
                q = np.float32(win[..., c].sum()) / cnt                  # f32 sums of bytes: exact below 2^24
                out[yy, xx, c] = np.uint8(min(max(np.trunc(q), 0), 255))
    return out


# ---- haze with density and airlight -------------------------------------------------------------------------------------------

def round_f32(q):
    """An exact rational rounded to the nearest f32, ties to even (one IEEE rounding; no overflow in the range used here)."""
    q = Fraction(q)
    if q < 0:
        return -round_f32(-q)
    if q == 0:
        return Fraction(0)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scale = Fraction(2) ** (max(e, -126) - 23)                        # ulp of the binade (subnormals: 2^-149)
    n = q / scale
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl * scale


def store_u8(v):
    """The library's float -> uchar: saturate, then truncate (NaN -> 0)."""
    if not v >= 0:
        return 0
    if v >= 255:
        return 255
    return int(v)


def haze_transmission(depth, beta, expf_det):
    """t = expf_det((float)((double)(-beta * d) / 255.0)) with the oracle's deterministic exp (orc_expf_vs_libm hook)."""
    arg = (np.float32(-beta) * depth.astype(np.float32)).astype(np.float64) / 255.0
    t, _ = expf_det(arg.astype(np.float32))
    return t


def haze_ex(orig, depth, beta, air, contract, expf_det):
    """out_c = (uchar)(t * o + (1 - t) * air_c), every f32 operation rounded once from its exact value (contract: t * o + w fused)."""
    t = haze_transmission(depth, beta, expf_det)
    out = np.empty_like(orig)
    memo = {}
    for c in range(3):
        ac = Fraction(int(air[c]))
        tc = t.reshape(-1); oc = orig[..., c].reshape(-1)
        keys = (tc.view(np.uint32).astype(np.uint64) << np.uint64(8)) | oc.astype(np.uint64)   # one key per (t, o) pair
        uk, inv = np.unique(keys, return_inverse=True)
        vals = np.empty(len(uk), np.uint8)
        first = np.zeros(len(uk), np.int64); first[inv[::-1]] = np.arange(len(inv))[::-1]
        for i, j in enumerate(first):
            tv, ov = float(tc[j]), int(oc[j])
            key = (tv, ov, int(air[c]), contract)
            if key not in memo:
                T = Fraction(tv)
                w = round_f32(round_f32(1 - T) * ac)
                v = round_f32(T * ov + w) if contract else round_f32(round_f32(T * ov) + w)
                memo[key] = store_u8(v)
            vals[i] = memo[key]
        out[..., c] = vals[inv].reshape(orig.shape[:2])
    return out
