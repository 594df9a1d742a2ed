"""Helpers shared by the -m gpu parity tests."""
import numpy as np

import realtimedepthdiffusion_amd as rt


def up(a, align=512):
    return rt.device_image(a, "cuda:0", align)


def down(t):
    return rt.to_host(t)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    if not np.array_equal(bits(got), bits(want)):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        n = int((bits(got) != bits(want)).sum())
        raise AssertionError(f"{what}: {n} of {got.size} values differ, max abs diff {np.nanmax(d):.3e}")


def assert_bit_equal_nan_aware(got, want, what=""):
    """Bit equality of two f32 arrays in which a NaN equals any NaN: x86, gfx950 and CUDA each produce a different default NaN, so a
    NaN's sign and payload are the one thing left out.  -0.0 and +0.0 stay distinct, and so do +inf and -inf."""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        finite = int((bad & np.isfinite(got) & np.isfinite(want)).sum())
        i = np.unravel_index(int(np.flatnonzero(bad)[0]), got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} values differ, {finite} of them finite on both sides; first at {tuple(int(k) for k in i)}: "
                             f"got {got[i]!r} (0x{int(bits(got)[i]):08x}), want {want[i]!r} (0x{int(bits(want)[i]):08x})")
