"""rtdd_simulate_relight_shadowed's restatements (tests/shadow_ref.py) pinned on the CPU: the vectorised one against the literal
per-pixel loop, the identities that follow from the header's rule, the known answer of a step in the height field; and the header
declares, the Python mirror names and both built libraries export the call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from relight_ref import DIRECTIONAL, POINT, light, relight
from shadow_ref import directional_step, relight_shadowed, relight_shadowed_literal, shadow, shadow_q, visibility

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _inputs(rows, cols, seed, nan=True):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    if nan:
        depth[rng.random((rows, cols)) < 0.05] = np.nan
    return orig, depth


def _lights(rows, cols, relief):
    """Both kinds; the point lights anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.125, diffuse=1.5)
    return [light(DIRECTIONAL, -1, -1, 1, **common),
            light(DIRECTIONAL, 3.5, -0.25, 0.5, color=(255, 128, 7), **common),
            light(DIRECTIONAL, 0.25, 2, 0.125, **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, -30.5, rows + 7.25, 200, anchorDepth=255, radius=500, color=(10, 200, 255), **common),
            light(POINT, cols // 3, rows - 1, 0.5, anchorX=cols // 3, anchorY=rows - 1, radius=3, **common)]


@pytest.mark.parametrize("relief", [0.0, 1.0, 64.0])
@pytest.mark.parametrize("softness", [0.0, 0.75])
def test_restatements_agree_on_random_maps(relief, softness):
    shaded = 0
    for i, (rows, cols) in enumerate([(1, 1), (3, 7), (6, 40), (9, 90)]):
        orig, depth = _inputs(rows, cols, 100 * i + int(relief) + 11)
        for L in _lights(rows, cols, relief):
            for steps in (1, 7, 64):
                S = shadow(steps, bias=0.5, softness=softness, strength=0.875)
                want = relight_shadowed_literal(orig, depth, L, S)
                assert np.array_equal(relight_shadowed(orig, depth, L, S), want), (rows, cols, L, S)
                shaded += int((want != relight(orig, depth, L)).any())
    assert (shaded > 0) == (relief > 0)                                 # a flat surface throws no shadow; a rough one does


def test_no_steps_and_no_strength_are_relight():
    orig, depth = _inputs(7, 60, 3)
    for L in _lights(7, 60, 2.0):
        want = relight(orig, depth, L)
        for S in (shadow(0, strength=1.0), shadow(64, strength=0.0), shadow(0, bias=3, softness=2, strength=0.5)):
            assert np.array_equal(relight_shadowed(orig, depth, L, S), want)
            assert np.array_equal(relight_shadowed_literal(orig, depth, L, S), want)
        assert not np.array_equal(relight_shadowed(orig, depth, L, shadow(64)), want)


def test_a_light_straight_above_shadows_nothing():
    orig, depth = _inputs(5, 30, 4)
    L = light(DIRECTIONAL, 0, 0, 2, relief=8, ambient=0.1, diffuse=1)
    assert directional_step(L) is None
    assert np.array_equal(relight_shadowed(orig, depth, L, shadow(64)), relight(orig, depth, L))
    assert np.array_equal(relight_shadowed_literal(orig, depth, L, shadow(64)), relight(orig, depth, L))


def test_constant_map_is_never_shadowed():
    """... by a light that does not stand below it (rise >= 0): every directional light, a point light anchored on the map or nearer."""
    orig, _ = _inputs(6, 50, 1)
    for d in (0.0, 77.25, 255.0, 300.0, np.nan):
        depth = np.full((6, 50), d, np.float32)
        lights = [L for L in _lights(6, 50, 64.0) if L["kind"] == DIRECTIONAL or L["anchorX"] >= 0]
        for L in lights + [light(POINT, 10, 3, 1e-3, anchorDepth=0, radius=5, relief=64), light(POINT, -7.5, 80, 30, anchorX=49, anchorY=5, radius=50, relief=3)]:
            for S in (shadow(64), shadow(64, softness=0.5), shadow(1024, bias=0.0, softness=1e-6)):
                assert (shadow_q(depth, L, S) == 0).all()
                assert np.array_equal(relight_shadowed(orig, depth, L, S), relight(orig, depth, L))


def test_mirror_symmetry():
    rows, cols = 5, 133
    orig, depth = _inputs(rows, cols, 4)
    of, df = np.ascontiguousarray(orig[:, ::-1]), np.ascontiguousarray(depth[:, ::-1])
    common = dict(relief=1.5, ambient=0.125, diffuse=1.0, color=(255, 200, 90))
    for S in (shadow(64), shadow(40, bias=1, softness=0.5, strength=0.75)):
        a = relight_shadowed(orig, depth, light(DIRECTIONAL, 1.25, -0.5, 0.75, **common), S)
        b = relight_shadowed(of, df, light(DIRECTIONAL, -1.25, -0.5, 0.75, **common), S)
        assert np.array_equal(b, a[:, ::-1]) and not np.array_equal(a, relight(orig, depth, light(DIRECTIONAL, 1.25, -0.5, 0.75, **common)))
        for x, ax in ((40.5, 17), (-20.0, 0), (cols + 3.0, cols - 1)):
            a = relight_shadowed(orig, depth, light(POINT, x, 2.5, 30, anchorX=ax, anchorY=3, radius=60, **common), S)
            b = relight_shadowed(of, df, light(POINT, cols - 1 - x, 2.5, 30, anchorX=cols - 1 - ax, anchorY=3, radius=60, **common), S)
            assert np.array_equal(b, a[:, ::-1])


def _step_map(rows=2, cols=200):
    depth = np.full((rows, cols), 255.0, np.float32)
    depth[:, :20] = 155.0                                               # a wall 100 high over x < 20, the floor at height 0
    return depth


def test_known_answer_the_shadow_of_a_step():
    """Light from the left at 45 degrees, (-1, 0, 1): sx = -1 and rise = 1 exactly.  The pixel at x sees the wall's nearest column 19 after
    k = x - 19 steps, where the ray stands at k: shadowed while k < 100, x = 20 .. 118; with 50 steps the march reaches it from x <= 69."""
    depth = _step_map()
    L = light(DIRECTIONAL, -1, 0, 1, relief=1, ambient=0, diffuse=1)
    assert directional_step(L) == (F(-1), F(0), F(1))
    hard = shadow(1024, bias=0, softness=0, strength=1)
    q = shadow_q(depth, L, hard)
    assert set(np.unique(q)) == {F(0), F(1)}
    assert np.array_equal(np.nonzero(q[0])[0], np.arange(20, 119)) and np.array_equal(q[0], q[1])
    assert np.array_equal(np.nonzero(shadow_q(depth, L, dict(hard, maxSteps=50))[0])[0], np.arange(20, 70))
    vis = visibility(depth, L, dict(hard, softness=0.5))[0]
    lit = np.empty(depth.shape, F)
    relight_shadowed_literal(np.zeros(depth.shape + (3,), np.uint8), depth, L, dict(hard, softness=0.5), vis_out=lit)
    assert np.array_equal(lit[0], vis)
    assert (vis[:20] == 1).all() and (vis[119:] == 1).all() and (vis[20:60] == 0).all()
    first = 20 + int(np.nonzero(vis[20:] > 0)[0][0])                    # (100 - k) / (0.5 k) < 1 from k = 67 on: x = 86
    assert first == 86
    edge = vis[first - 1:119 + 1]                                       # from the last fully dark column to the first lit one
    assert edge[0] == 0 and edge[-1] == 1 and len(edge) > 3 and (np.diff(edge) > 0).all()
    # the bytes: a shadowed pixel keeps the ambient term only
    orig = np.full(depth.shape + (3,), 200, np.uint8)
    out = relight_shadowed(orig, depth, dict(L, ambient=0.25), hard)
    assert (out[:, 20:119] == 50).all() and (out[:, 119:] == relight(orig, depth, dict(L, ambient=0.25))[:, 119:]).all()
    half = relight_shadowed(orig, depth, L, dict(hard, strength=0.5))
    assert (half[:, 30:110] == relight(orig, depth, L)[:, 30:110] // 2).all()


def test_bias_lifts_the_ray():
    depth = _step_map()
    L = light(DIRECTIONAL, -1, 0, 1, relief=1, ambient=0, diffuse=1)
    q = shadow_q(depth, L, shadow(1024, bias=40))
    assert np.array_equal(np.nonzero(q[0])[0], np.arange(20, 79))       # occ = 100 - (40 + k) > 0: k < 60
    assert (shadow_q(depth, L, shadow(1024, bias=100)) == 0).all()


def test_point_light_straight_above_a_pixel_leaves_it_lit():
    """Two pits (height 0) in a plateau 1020 high, a light half a pixel above the floor of the first: m < 1 there, no step is taken and the
    pit is lit, although every neighbour towers over the light; the second pit marches into the plateau at its first step."""
    depth = np.zeros((9, 41), np.float32)
    depth[4, 20] = depth[4, 24] = 255.0
    for x, y in ((20.0, 4.0), (20.5, 3.75), (19.25, 4.5)):             # m = 0, 0.5, 0.75 at (20, 4)
        L = light(POINT, x, y, 0.5, anchorDepth=255, radius=50, relief=4)
        for S in (shadow(64), shadow(1024, softness=0.25)):
            q = shadow_q(depth, L, S)
            assert q[4, 20] == 0 and q[4, 24] == 1
    L = light(POINT, 21.0, 4.0, 0.5, anchorDepth=255, radius=50, relief=4)
    assert shadow_q(depth, L, shadow(64))[4, 20] == 1                   # m == 1: one step, into the plateau


def test_point_light_march_never_passes_the_light():
    """A wall BEHIND the light, as seen from the pixel, throws no shadow on it: n = min(maxSteps, (int)m)."""
    rows, cols = 3, 120
    depth = np.full((rows, cols), 255.0, np.float32)
    depth[:, :10] = 0.0                                                 # a wall 255 high at x < 10
    L = light(POINT, 30.0, 1.0, 5.0, anchorDepth=255, radius=100, relief=1)
    q = shadow_q(depth, L, shadow(1024))
    assert (q[:, 10:] == 0).all()                                       # the light stands between them and the wall
    far = light(POINT, -20.0, 1.0, 5.0, anchorDepth=255, radius=100, relief=1)
    qf = shadow_q(depth, far, shadow(1024))
    assert (qf[1, 10:100] == 1).all()                                   # the same wall between pixel and light
    lit = np.empty(depth.shape, F)
    relight_shadowed_literal(np.zeros((rows, cols, 3), np.uint8), depth, L, shadow(1024), vis_out=lit)
    assert (lit[:, 10:] == 1).all()


def test_header_declares_and_both_libraries_export_the_call():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert re.search(r"#define RTDD_VERSION 230\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"typedef struct rtdd_shadow \{(.*?)\} rtdd_shadow;", code, flags=re.S)
    assert m
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int maxSteps; float bias; float softness; float strength;"
    assert re.search(r"int rtdd_simulate_relight_shadowed\(rtdd_ctx \*ctx,[^;]*int rows, int cols, const rtdd_light \*light, "
                     r"const rtdd_shadow \*shadow\s*\);", code)
    assert "rtdd_simulate_relight_shadowed" in rt.C_ABI_SYMBOLS and hasattr(rt.Context, "simulate_relight_shadowed")
    assert [n for n, _ in rt.Shadow._fields_] == ["maxSteps", "bias", "softness", "strength"]
    assert C.sizeof(rt.Shadow) == 16 and C.sizeof(rt.Light) == 48
    so = rt.build()
    for lib in (so, os.path.join(os.path.dirname(so), "librtdd_acq.so")):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        assert "rtdd_simulate_relight_shadowed" in {line.split()[-1] for line in out.splitlines() if " T " in line}, lib
        # ... and the library holds the kernel's translation unit too: it loads with every symbol bound (a fresh process, no GPU needed)
        code = "import ctypes, os; ctypes.CDLL(%r, mode=os.RTLD_NOW); print('loaded')" % lib
        r = subprocess.run([sys.executable, "-c", "import torch\n" + code], capture_output=True, text=True)
        assert r.returncode == 0 and "loaded" in r.stdout, lib + ": " + r.stderr
