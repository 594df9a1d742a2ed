"""rtdd_simulate_ambient_occlusion's restatements (tests/ao_ref.py) pinned on the CPU: the vectorised one against the literal per-pixel
loop, the identities that follow from the header's rule, the known answer of a wall; and the header declares, the Python mirror names
and both built libraries export the call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from ao_ref import MAP, SHADE, ambient, ambient_literal, inv_step, occluded, occluded_literal, occlusion
from relight_ref import DIRECTIONAL, POINT, light, relight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(1, 1), (3, 7), (6, 40), (9, 90)]


def _inputs(rows, cols, seed, nan=True):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    if nan:
        depth[rng.random((rows, cols)) < 0.05] = np.nan
    return orig, depth


def _lights(rows, cols, relief):
    """No light, a directional light, point lights anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.75, diffuse=1.5)
    return [None,
            light(DIRECTIONAL, 3.5, -0.25, 0.5, color=(255, 128, 7), **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, cols // 3, rows - 1, 0.5, anchorX=cols // 3, anchorY=rows - 1, radius=3, color=(10, 200, 255), **common)]


@pytest.mark.parametrize("relief", [0.0, 1.0, 64.0])
@pytest.mark.parametrize("radius", [1, 7, 64])
def test_restatements_agree_on_random_maps(relief, radius):
    darkened = 0
    for i, (rows, cols) in enumerate(SHAPES):
        orig, depth = _inputs(rows, cols, 100 * i + int(relief) + radius)
        for directions in (4, 8):
            A = occlusion(SHADE, directions, radius, relief, bias=0.5, strength=0.875)
            ao = ambient_literal(depth, A)
            assert np.array_equal(ambient(depth, A), ao), (rows, cols, A)
            assert (ao >= 0).all() and (ao <= 1).all()
            darkened += int((ao < 1).any())
            for L in _lights(rows, cols, relief):
                assert np.array_equal(occluded(orig, depth, A, L), occluded_literal(orig, depth, A, L, ao)), (rows, cols, A, L)
            M = dict(A, mode=MAP)
            assert np.array_equal(occluded(orig, depth, M), occluded_literal(orig, depth, M, None, ao)), (rows, cols, M)
    assert (darkened > 0) == (relief > 0)                               # a flat surface occludes nothing; a rough one does


def test_a_band_of_rows_is_the_images_rows():
    orig, depth = _inputs(40, 50, 8)
    L = light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.5, diffuse=1)
    for A in (occlusion(SHADE, 8, 16, 2.0, 0.25, 1.0), occlusion(SHADE, 4, 64, 2.0, 0.0, 0.5)):
        assert np.array_equal(occluded(orig, depth, A, L, rows=(7, 29)), occluded(orig, depth, A, L)[7:29])
        assert np.array_equal(occluded(orig, depth, dict(A, mode=MAP), rows=(0, 3)), occluded(orig, depth, dict(A, mode=MAP))[0:3])


def test_identities():
    """radius 0, strength 0, relief 0 or a constant map: the original, relight's bytes under a light, a map of 255."""
    rows, cols = 7, 60
    orig, depth = _inputs(rows, cols, 3)
    const = np.full((rows, cols), 93.5, np.float32)
    cases = [(depth, occlusion(SHADE, 8, 0, 2.0, 0.0, 1.0)), (depth, occlusion(SHADE, 4, 16, 2.0, 0.0, 0.0)),
             (depth, occlusion(SHADE, 8, 16, 0.0, 0.0, 1.0)), (const, occlusion(SHADE, 8, 16, 2.0, 0.0, 1.0)),
             (np.full((rows, cols), np.nan, np.float32), occlusion(SHADE, 4, 64, 64.0, 0.0, 1.0))]
    for d, A in cases:
        for f in (occluded, occluded_literal):
            assert np.array_equal(f(orig, d, A), orig), A
            assert (f(orig, d, dict(A, mode=MAP)) == 255).all(), A
            for L in _lights(rows, cols, A["relief"])[1:]:
                assert np.array_equal(f(orig, d, A, L), relight(orig, d, L)), (A, L)
    A = occlusion(SHADE, 8, 16, 2.0, 0.0, 1.0)                          # ... and a rough map under the same settings is occluded
    assert not np.array_equal(occluded(orig, depth, A), orig)
    L = _lights(rows, cols, 2.0)[1]
    assert not np.array_equal(occluded(orig, depth, A, L), relight(orig, depth, L))


def test_the_tables_are_rounded_once_from_double():
    assert inv_step(0, 1) == F(1) and inv_step(2, 4) == F(0.25) and inv_step(6, 3) == F(1.0 / 3.0)
    assert inv_step(1, 1) == F(0.7071067811865475) and inv_step(7, 64) == F(1.0 / (64.0 * 2.0 ** 0.5))


def _wall(rows, cols, x0, a, b):
    depth = np.full((rows, cols), a, np.float32)
    depth[:, x0:] = b
    return depth


@pytest.mark.parametrize("radius", [1, 5, 64])
def test_known_answer_the_foot_of_a_wall(radius):
    """A map that is a for x < x0 and b < a for x >= x0: a wall nearer on the right.  With 4 directions the pixel at x0 - 1 on an interior
    row sees it at k = 1 in direction 0 (inv = 1) and nothing above its own plane elsewhere; the pixel at x0 stands on the wall."""
    rows, cols, x0, a, b = 5, 40, 17, 200.0, 120.5
    for r, beta in ((1.0, 0.0), (2.5, 3.0), (64.0, 0.25)):
        depth = _wall(rows, cols, x0, a, b)
        A = occlusion(SHADE, 4, radius, r, beta, 1.0)
        t = F(F(F(r) * F(F(255) - F(b))) - F(F(r) * F(F(255) - F(a)))) - F(beta)
        assert t.dtype == F and t > 0
        occ0 = F(t / np.sqrt(F(F(1) + F(t * t))))
        want = F(F(1) - F(F(1) * F(occ0 * F(0.25))))
        occ = np.full((rows, cols, 8), np.nan, F)
        ao_l = ambient_literal(depth, A, occ_out=occ)
        ao = ambient(depth, A)
        assert np.array_equal(ao, ao_l)
        y = rows // 2
        assert occ[y, x0 - 1, 0] == occ0 and (occ[y, x0 - 1, [2, 4, 6]] == 0).all()
        assert ao[y, x0 - 1] == want and ao[y, x0] == 1
        assert (ao[:, x0:] == 1).all()                                  # nothing rises above the wall's top
        # farther from the wall the tangent falls as 1 / k: the occlusion fades and ends where the radius does
        seen = ao[y, :x0] < 1
        first = max(x0 - radius, 0)
        assert np.array_equal(np.nonzero(seen)[0], np.arange(first, x0)) and (np.diff(ao[y, first:x0]) <= 0).all()
        assert radius == 1 or ao[y, first] > ao[y, x0 - 1]
        orig = np.full((rows, cols, 3), 200, np.uint8)
        out = occluded(orig, depth, A)
        assert (out[y, x0 - 1] == int(F(200) * want)).all() and (out[:, x0:] == 200).all()
        assert (occluded(orig, depth, dict(A, mode=MAP))[y, x0 - 1] == int(F(255) * want)).all()


def test_bias_and_strength():
    depth = _wall(5, 40, 17, 200.0, 120.0)                              # a step of 80 at relief 1
    assert (ambient(depth, occlusion(SHADE, 8, 16, 1.0, 80.0, 1.0)) == 1).all()       # the horizon does not clear the bias
    assert (ambient(depth, occlusion(SHADE, 8, 16, 1.0, 79.0, 1.0)) < 1).any()
    full, half = ambient(depth, occlusion(SHADE, 8, 16, 1.0, 0.0, 1.0)), ambient(depth, occlusion(SHADE, 8, 16, 1.0, 0.0, 0.5))
    assert np.array_equal(half < 1, full < 1) and (half[full < 1] > full[full < 1]).all()
    assert np.abs((F(1) - half) - (F(1) - full) * F(0.5)).max() <= 2 * np.finfo(F).eps      # (halving is exact; 1 - . rounds, three times)
    # a pit one pixel wide between two walls: all eight horizons stand high, the occlusion nearly complete
    pit = np.zeros((9, 9), np.float32)
    pit[4, 4] = 255.0
    ao = ambient(pit, occlusion(SHADE, 8, 4, 64.0, 0.0, 1.0))
    assert ao[4, 4] < 0.001 and (ao[pit == 0] == 1).all()


def test_mirror_symmetry():
    """Mirroring the map mirrors the occlusion: the directions come in mirrored pairs that are added in another order, so the sums agree
    to rounding only.  Eight directions: 7 additions of partial sums below 8, each off by at most ulp(4) / 2 = 2 eps, in either order, times
    1 / 8: 3.5 eps, and two more roundings of values below 1 -- 8 eps covers it; four directions: 2 * 3 * eps / 4 and the same two."""
    _, depth = _inputs(6, 70, 4)
    A = occlusion(SHADE, 8, 7, 1.5, 0.25, 1.0)
    a, b = ambient(depth, A), ambient(np.ascontiguousarray(depth[:, ::-1]), A)[:, ::-1]
    assert np.abs(a - b).max() <= 8 * np.finfo(F).eps
    A4 = dict(A, directions=4)                                          # ((occ_0 + occ_2) + occ_4) + occ_6 against ((occ_4 + occ_2) + occ_0) + occ_6
    assert np.abs(ambient(depth, A4) - ambient(np.ascontiguousarray(depth[:, ::-1]), A4)[:, ::-1]).max() <= 4 * np.finfo(F).eps


def test_header_declares_and_both_libraries_export_the_call():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert re.search(r"#define RTDD_VERSION 230\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"typedef struct rtdd_ambient_occlusion \{(.*?)\} rtdd_ambient_occlusion;", code, flags=re.S)
    assert m
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int mode; int directions; int radius; float relief; float bias; float strength;"
    assert re.search(r"enum rtdd_ao_mode \{ RTDD_AO_SHADE = 0, RTDD_AO_MAP = 1 \};", code)
    assert re.search(r"int rtdd_simulate_ambient_occlusion\(rtdd_ctx \*ctx,[^;]*int rows, int cols, const rtdd_ambient_occlusion \*ao,\s*"
                     r"const rtdd_light \*light\s*\);", code)
    assert "rtdd_simulate_ambient_occlusion" in re.search(r"a host finds them by symbol.*?\*/", header, flags=re.S).group(0)
    assert "rtdd_simulate_ambient_occlusion" in rt.C_ABI_SYMBOLS and hasattr(rt.Context, "simulate_ambient_occlusion")
    assert [n for n, _ in rt.AmbientOcclusion._fields_] == ["mode", "directions", "radius", "relief", "bias", "strength"]
    assert C.sizeof(rt.AmbientOcclusion) == 24 and C.sizeof(rt.Light) == 48 and (rt.AO_SHADE, rt.AO_MAP) == (SHADE, MAP)
    so = rt.build()
    for lib in (so, os.path.join(os.path.dirname(so), "librtdd_acq.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        assert "rtdd_simulate_ambient_occlusion" in {line.split()[-1] for line in out.splitlines() if " T " in line}, lib
        # ... and the library holds the kernel's translation unit too: it loads with every symbol bound (a fresh process, no GPU needed)
        code = "import ctypes, os; ctypes.CDLL(%r, mode=os.RTLD_NOW); print('loaded')" % lib
        r = subprocess.run([sys.executable, "-c", "import torch\n" + code], capture_output=True, text=True)
        assert r.returncode == 0 and "loaded" in r.stdout, lib + ": " + r.stderr
