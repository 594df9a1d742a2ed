"""rtdd_simulate_stereo's restatements (tests/stereo_ref.py) pinned on the CPU: the vectorised one against the literal per-pixel loop,
known answers, mirror symmetry, the anaglyph's channels, the hole-run bound the kernel's halo rests on (DESIGN.md "Stereo"); and the
header declares, the Python mirror names and both built libraries export the call."""
import os
import re
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from stereo_ref import ANAGLYPH, VIEW, hole_runs, shifts, stereo, stereo_literal, stereo_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(rows, cols, seed, nan=True):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    if nan:
        depth[rng.random((rows, cols)) < 0.05] = np.nan
    return orig, depth


@pytest.mark.parametrize("D", [-256, -37, -5, -1, 0, 1, 2, 19, 64, 256])
def test_restatements_agree_on_random_maps(D):
    for i, (rows, cols) in enumerate([(1, 1), (2, 7), (3, 40), (2, 97), (2, 300)]):
        orig, depth = _inputs(rows, cols, 100 * i + D + 300)
        for mode in (VIEW, ANAGLYPH):
            for z0 in (0.0, 127.5, 255.0, 63.75):
                assert np.array_equal(stereo(orig, depth, D, z0, mode=mode), stereo_literal(orig, depth, D, z0, mode=mode)), (rows, cols, z0, mode)
            zx, zy = cols // 2, rows - 1
            assert np.array_equal(stereo(orig, depth, D, zx=zx, zy=zy, mode=mode), stereo_literal(orig, depth, D, zx=zx, zy=zy, mode=mode))


def test_exact_half_quotients_round_half_to_even():
    # D = 2: d' - z0 = 63.75 gives q = 0.5 -> 0, 191.25 gives 1.5 -> 2, -63.75 gives -0.5 -> 0; NaN is depth 0
    d = np.array([[63.75, 191.25, 0.0, np.nan, 255.0]], np.float32)
    assert shifts(d, 2, 0.0).tolist() == [[0, 2, 0, 0, 2]]
    assert shifts(np.array([[0.0]], np.float32), 2, 63.75).tolist() == [[0]]
    rng = np.random.default_rng(1)
    row = rng.choice(np.array([63.75, 191.25, 127.5, 0.0], np.float32), (3, 64))
    orig = rng.integers(0, 256, (3, 64, 3), dtype=np.uint8)
    for D in (2, -2, 6):
        assert np.array_equal(stereo(orig, row, D), stereo_literal(orig, row, D))


def test_zero_disparity_is_the_identity():
    orig, depth = _inputs(4, 50, 2)
    for mode in (VIEW, ANAGLYPH):
        assert np.array_equal(stereo(orig, depth, 0, 77.0, mode=mode), orig)


def test_constant_depth_is_a_translation_with_border_filling():
    orig, _ = _inputs(3, 20, 3)
    far = np.full((3, 20), 255.0, np.float32)
    v = stereo(orig, far, 5, 0.0)                   # s = +5 everywhere: the view moves right, the left border copies target 5
    assert np.array_equal(v[:, 5:], orig[:, :15])
    assert np.array_equal(v[:, :5], np.repeat(orig[:, :1], 5, 1))
    v = stereo(orig, far, -5, 0.0)                  # s = -5: moves left, the right border copies target 14 (the background side, left)
    assert np.array_equal(v[:, :15], orig[:, 5:])
    assert np.array_equal(v[:, 15:], np.repeat(orig[:, 19:], 5, 1))
    v = stereo(orig, np.zeros((3, 20), np.float32), 5, 255.0)   # s = -5 with D > 0: no filled target on the right, the left side fills
    assert np.array_equal(v[:, :15], orig[:, 5:])
    assert np.array_equal(v[:, 15:], np.repeat(orig[:, 19:], 5, 1))


def test_near_square_on_far_background_leaves_a_background_hole():
    rows, cols = 6, 40
    orig = np.zeros((rows, cols, 3), np.uint8)
    orig[:] = (10, 20, 30)                                             # background
    orig[1:5, 10:20] = np.arange(10, dtype=np.uint8)[:, None] * 20 + 50  # the square, a ramp
    depth = np.full((rows, cols), 255.0, np.float32)
    depth[1:5, 10:20] = 0.0
    v = stereo(orig, depth, 8, 255.0)               # the far plane on the screen: the near square moves 8 left
    assert np.array_equal(v[[0, 5]], orig[[0, 5]])
    assert np.array_equal(v[1:5, 2:12], orig[1:5, 10:20])              # the square, in front of the background it covers
    assert (v[1:5, 12:20] == (10, 20, 30)).all()                       # the hole: 8 wide, the background's colour from the right
    assert np.array_equal(v[1:5, :2], orig[1:5, :2]) and np.array_equal(v[1:5, 20:], orig[1:5, 20:])
    _, filled = stereo_sources(depth, 8, 255.0)
    assert [r[:2] for r in hole_runs(filled[2])] == [(12, 8)]


@pytest.mark.parametrize("D", [-200, -19, 1, 19, 256])
def test_mirror_symmetry(D):
    orig, depth = _inputs(5, 333, 4)
    for z0 in (0.0, 127.5, 255.0):
        assert np.array_equal(stereo(orig[:, ::-1], np.ascontiguousarray(depth[:, ::-1]), -D, z0), stereo(orig, depth, D, z0)[:, ::-1])


@pytest.mark.parametrize("D", [19, -19])
def test_anaglyph_channels(D):
    orig, depth = _inputs(4, 120, 5)
    v, a = stereo(orig, depth, D, 100.0), stereo(orig, depth, D, 100.0, mode=ANAGLYPH)
    if D >= 0:
        assert np.array_equal(a[..., :2], v[..., :2]) and np.array_equal(a[..., 2], orig[..., 2])
    else:
        assert np.array_equal(a[..., :2], orig[..., :2]) and np.array_equal(a[..., 2], v[..., 2])
    assert not np.array_equal(v, orig)


def test_hole_runs_are_bounded():
    """Every hole run but a whole-row one is at most |D| + 1 long, and a row without a filled target has cols <= |D| + 1."""
    rng = np.random.default_rng(6)
    for it in range(1500):
        cols = int(rng.integers(1, 700)); D = int(rng.integers(-256, 257)); z0 = float(rng.uniform(0, 255))
        if it % 3 == 0:
            depth = rng.uniform(-20, 280, (1, cols)).astype(np.float32)
        else:
            w = int(rng.integers(1, 2 * abs(D) + 3))
            depth = np.repeat(rng.choice([0.0, 255.0], cols // w + 1), w)[None, :cols].astype(np.float32)
        s = shifts(depth, D, z0)
        assert s.max() - s.min() <= abs(D) + 1 and np.abs(s).max() <= abs(D)
        _, filled = stereo_sources(depth, D, z0)
        for start, length, whole in hole_runs(filled[0]):
            if whole:
                assert cols <= abs(D) + 1, (cols, D)
            else:
                assert length <= abs(D) + 1, (cols, D, z0, start, length)


def test_header_declares_and_both_libraries_export_the_call():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"enum rtdd_stereo_mode \{ RTDD_STEREO_VIEW = 0, RTDD_STEREO_ANAGLYPH = 1 \};", code)
    assert re.search(r"int rtdd_simulate_stereo\(rtdd_ctx \*ctx,[^;]*int rows, int cols, int disparity, float zeroParallaxDepth, int zeroX, "
                     r"int zeroY, int mode\);", code)
    assert "rtdd_simulate_stereo" in rt.C_ABI_SYMBOLS
    assert hasattr(rt.Context, "simulate_stereo") and (rt.STEREO_VIEW, rt.STEREO_ANAGLYPH) == (0, 1)
    so = rt.build()
    for lib in (so, os.path.join(os.path.dirname(so), "librtdd_acq.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        assert "rtdd_simulate_stereo" in {line.split()[-1] for line in out.splitlines() if " T " in line}, lib
