"""rtdd_simulate_parallax's restatements (tests/parallax_ref.py) pinned on the CPU: the vectorised one against the literal per-pixel
loop, the horizontal case against the stereo restatement (tests/stereo_ref.py), the identities, known answers, the dtype of every f32
intermediate; and the header declares, the Python mirror names and both built libraries export the call."""
import os
import re
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from parallax_ref import EMPTY, intermediates, parallax, parallax_literal, scatter
from stereo_ref import stereo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 64), (5, 97), (9, 300)]


def _maps(rows, cols, seed):
    rng = np.random.default_rng(seed)
    rnd = rng.uniform(-20, 280, (rows, cols)).astype(np.float32)
    step = np.where(np.arange(cols)[None, :] < cols // 2, 20.0, 230.0).astype(np.float32).repeat(rows, 0)
    ramp = np.broadcast_to(np.linspace(0, 255, cols, dtype=np.float32), (rows, cols)).copy()
    const = np.full((rows, cols), 99.0, np.float32)
    return {"random": rnd, "step": step, "ramp": ramp, "constant": const}


def _orig(rows, cols, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_horizontal_case_is_the_stereo_view(shape):
    rows, cols = shape
    orig = _orig(rows, cols)
    for name, depth in _maps(rows, cols, rows + cols).items():
        for D in (-256, -37, 0, 1, 19, 256):
            for z0 in (0.0, 127.5, 255.0):
                assert np.array_equal(parallax(orig, depth, D, 0, 0.0, z0), stereo(orig, depth, D, z0)), (name, D, z0)
    depth = _maps(rows, cols, 1)["random"]
    depth[0, 3] = np.nan
    zx, zy = cols // 2, rows - 1
    assert np.array_equal(parallax(orig, depth, 19, zx=zx, zy=zy), stereo(orig, depth, 19, zx=zx, zy=zy))
    assert np.array_equal(parallax(orig, depth, -19, 0, -0.0, 60.0), stereo(orig, depth, -19, 60.0))        # a dolly of -0 is no dolly


VIEWS = [(0, 7, 0.0), (5, -3, 0.0), (-256, 256, 0.0), (0, 0, 0.4), (0, 0, -0.4), (3, -2, 0.25), (-7, 1, -1.0), (1, 0, 0.0), (0, -1, 0.0)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 1), (6, 11), (9, 23)])
def test_restatements_agree(shape):
    rows, cols = shape
    orig = _orig(rows, cols, 3)
    for name, depth in _maps(rows, cols, 7 * rows + cols).items():
        if name == "random":
            depth[np.random.default_rng(5).random((rows, cols)) < 0.1] = np.nan
            depth[0, 0] = np.inf; depth[-1, -1] = -np.inf; depth[rows // 2, cols // 2] = -0.0
        for sx, sy, dolly in VIEWS:
            span = max(rows - 1, cols - 1, 1)
            dolly = dolly * min(1.0, 512.0 / span)
            for z0 in (0.0, 127.5, 255.0):
                assert np.array_equal(parallax(orig, depth, sx, sy, dolly, z0), parallax_literal(orig, depth, sx, sy, dolly, z0)), (name, sx, sy, dolly, z0)
        zx, zy = cols - 1, rows // 2
        assert np.array_equal(parallax(orig, depth, 4, -5, 0.3, zx=zx, zy=zy), parallax_literal(orig, depth, 4, -5, 0.3, zx=zx, zy=zy)), name


def test_identities():
    rows, cols = 8, 40
    orig = _orig(rows, cols, 4)
    depth = _maps(rows, cols, 2)["random"]
    for z0 in (0.0, 100.0):
        assert np.array_equal(parallax(orig, depth, 0, 0, 0.0, z0), orig)
    const = np.full((rows, cols), 99.0, np.float32)
    for view in VIEWS:
        assert np.array_equal(parallax(orig, const, *view, z0=99.0), orig), view
        assert np.array_equal(parallax(orig, const, *view, zx=3, zy=2), orig), view
    assert not np.array_equal(parallax(orig, depth, 0, 5, 0.0, 100.0), orig)
    assert not np.array_equal(parallax(orig, depth, 0, 0, 0.5, 100.0), orig)


def test_vertical_shift_is_the_horizontal_one_transposed():
    rows, cols = 33, 21
    orig, depth = _orig(rows, cols, 6), _maps(rows, cols, 3)["random"]
    ot, dt = np.ascontiguousarray(orig.transpose(1, 0, 2)), np.ascontiguousarray(depth.T)
    for D in (-30, 7, 256):
        _, same = scatter(depth, 0, D, 0.0, 120.0)
        assert same.max() <= 1                          # equal depths shift alike within a column: no tie, the index order cannot matter
        a = parallax(orig, depth, 0, D, 0.0, 120.0)
        assert np.array_equal(a, parallax(ot, dt, D, 0, 0.0, 120.0).transpose(1, 0, 2))
        assert np.array_equal(a, stereo(ot, dt, D, 120.0).transpose(1, 0, 2))


def test_constant_depth_translates_and_fills_from_the_background_side():
    orig = _orig(12, 20, 7)
    far = np.full((12, 20), 255.0, np.float32)
    v = parallax(orig, far, 5, 3, 0.0, 0.0)             # every source moves by (+5, +3)
    assert np.array_equal(v[3:, 5:], orig[:-3, :-5])
    # a hole at (x < 5 or y < 3) marches along (5, 3) / 5: p = t + (k, rint(0.6 k)); the first filled target on it
    for (y, x) in ((0, 0), (2, 4), (7, 2), (1, 12)):
        k = 1
        while not (x + k >= 5 and y + int(np.rint(np.float32(k) * (np.float32(3) / np.float32(5)))) >= 3):
            k += 1
        py, px = y + int(np.rint(np.float32(k) * (np.float32(3) / np.float32(5)))), x + k
        assert np.array_equal(v[y, x], orig[py - 3, px - 5]), (y, x)


def test_forward_dolly_on_a_near_plane_spreads_from_the_centre():
    rows, cols = 9, 9
    orig = _orig(rows, cols, 8)
    near = np.zeros((rows, cols), np.float32)
    # ax = -0.5 (x - 4) and d' - z0 = -255: sx = rint(0.5 (x - 4)), half to even -- -2 -2 -1 0 0 0 1 2 2 for x = 0 .. 8.  In the middle
    # row (ay = 0) the sources 2 3 4 5 6 fill the targets 1 3 4 5 7; the holes 0 and 2 (ax > 0) take their right neighbour's view, the
    # holes 6 and 8 (ax < 0) their left neighbour's: the background side is towards the centre
    v = parallax(orig, near, 0, 0, 0.5, 255.0)
    assert np.array_equal(v[4], orig[4, [2, 2, 3, 3, 4, 5, 5, 6, 6]])
    assert np.array_equal(v[:, 4], orig[[2, 2, 3, 3, 4, 5, 5, 6, 6], 4])
    assert np.array_equal(v, parallax_literal(orig, near, 0, 0, 0.5, 255.0))
    # a far plane under the same dolly contracts towards the centre: the sources of columns and rows 1, 2, 3 share the targets of column and row 3
    far = np.full((rows, cols), 255.0, np.float32)
    w = parallax(orig, far, 0, 0, 0.5, 0.0)
    assert np.array_equal(w, parallax_literal(orig, far, 0, 0, 0.5, 0.0))
    assert np.array_equal(w[4, 4], orig[4, 4]) and np.array_equal(w[3, 3], orig[1, 1]) and np.array_equal(w[4, 3], orig[4, 1])       # equal depths: the smallest source index


def test_ties_go_to_the_smallest_source_index():
    rows, cols = 11, 13
    orig = _orig(rows, cols, 9)
    const = np.full((rows, cols), 200.0, np.float32)
    keys, same = scatter(const, 0, 0, 1.0, 0.0)        # a contracting dolly on a far plane: several equal-depth sources per target
    assert (same >= 2).any()
    lit = parallax_literal(orig, const, 0, 0, 1.0, 0.0)
    assert np.array_equal(parallax(orig, const, 0, 0, 1.0, 0.0), lit)
    flat = orig.reshape(-1, 3)
    ys, xs = np.nonzero(same >= 2)
    for y, x in zip(ys, xs):
        f32, sx, sy = intermediates(const, 0, 0, 1.0, 0.0)
        yy, xx = np.mgrid[0:rows, 0:cols]
        cands = (yy * cols + xx)[(xx + sx == x) & (yy + sy == y)]
        assert len(cands) >= 2 and np.array_equal(lit[y, x], flat[cands.min()])


def test_every_f32_intermediate_is_float32():
    depth = _maps(5, 17, 1)["random"]
    for kw in (dict(shiftX=3, shiftY=-4, dolly=0.5, z0=10.0), dict(shiftX=256, zx=2, zy=1), dict(dolly=-2.0)):
        f32, sx, sy = intermediates(depth, **kw)
        for name, v in f32.items():
            assert v.dtype == np.float32, name
        assert np.abs(sx).max() <= 512 and np.abs(sy).max() <= 512
    # the bound of the header at its edge: |shift| = 256, |dolly| * span / 2 = 256
    f32, sx, sy = intermediates(np.array([[0.0, 255.0] * 50 + [0.0]], np.float32), 256, -256, 256.0 / 50.0, 255.0)
    assert np.abs(f32["ax"]).max() <= 512 and np.abs(f32["ay"]).max() <= 512 and np.abs(sx).max() <= 512


def test_header_declares_and_both_libraries_export_the_call():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct rtdd_parallax \{\s*int\s+shiftX, shiftY;\s*float dolly;\s*float zeroParallaxDepth;\s*int\s+zeroX, zeroY;\s*\} rtdd_parallax;", code)
    assert re.search(r"int rtdd_simulate_parallax\(rtdd_ctx \*ctx,[^;]*int rows, int cols, const rtdd_parallax \*view\s*\);", code)
    assert "#define RTDD_VERSION 230" in header
    assert "rtdd_simulate_parallax" in rt.C_ABI_SYMBOLS and hasattr(rt.Context, "simulate_parallax")
    assert [f[0] for f in rt.Parallax._fields_] == ["shiftX", "shiftY", "dolly", "zeroParallaxDepth", "zeroX", "zeroY"]
    import ctypes
    assert ctypes.sizeof(rt.Parallax) == 24
    so = rt.build()
    for lib in (so, os.path.join(os.path.dirname(so), "librtdd_acq.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        assert "rtdd_simulate_parallax" in {line.split()[-1] for line in out.splitlines() if " T " in line}, lib
