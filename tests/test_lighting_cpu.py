"""rtdd_simulate_lighting's restatements (tests/lighting_ref.py) pinned on the CPU: the vectorised one against the literal per-pixel
loop, the three identities of the header against the restatements of the calls it fuses, and that it is neither of them where both
terms show; and the header declares, the Python mirror names and the built library exports the call."""
import os
import re
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from ao_ref import SHADE, occluded, occlusion
from lighting_ref import lighting, lighting_literal
from relight_ref import DIRECTIONAL, POINT, light, relight
from shadow_ref import relight_shadowed, shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 37), (23, 1), (23, 131)]


def _inputs(rows, cols, seed):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    depth[rng.random((rows, cols)) < 0.05] = np.nan
    return orig, depth


def _lights(rows, cols, relief):
    """A directional light; point lights inside the image, anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.75, diffuse=1.5)
    return [light(DIRECTIONAL, -1, -1, 1, color=(255, 128, 7), **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, cols // 3, rows - 1, 0.5, anchorX=cols // 3, anchorY=rows - 1, radius=3, color=(10, 200, 255), **common)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatements_agree_on_random_maps(shape):
    rows, cols = shape
    orig, depth = _inputs(rows, cols, rows * 1000 + cols)
    for i, L in enumerate(_lights(rows, cols, 1.5)):
        S = shadow(64, bias=0.25, softness=0.5 * (i % 2), strength=0.875)
        A = occlusion(SHADE, 8 if i != 1 else 4, (16, 5, 64)[i], 1.5, bias=0.25, strength=0.875)
        assert np.array_equal(lighting(orig, depth, L, S, A), lighting_literal(orig, depth, L, S, A)), (shape, L, S, A)


def test_a_band_of_rows_is_the_images_rows():
    orig, depth = _inputs(40, 50, 8)
    for L in _lights(40, 50, 2.0)[:2]:
        S, A = shadow(30, softness=0.5), occlusion(SHADE, 8, 9, 2.0, 0.5, 1.0)
        assert np.array_equal(lighting(orig, depth, L, S, A, rows=(11, 29)), lighting(orig, depth, L, S, A)[11:29])


@pytest.mark.parametrize("shape", [(23, 131), (9, 67), (1, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_three_identities(shape):
    rows, cols = shape
    orig, depth = _inputs(rows, cols, 77 + cols)
    S, A = shadow(64, bias=0.125, softness=0.5, strength=0.75), occlusion(SHADE, 8, 16, 1.5, 0.25, 0.875)
    for L in _lights(rows, cols, 1.5):
        for S0 in (dict(S, maxSteps=0), dict(S, strength=0.0)):            # no shadows: ambient occlusion under the light
            assert np.array_equal(lighting(orig, depth, L, S0, A), occluded(orig, depth, A, L)), (L, S0)
        for A0 in (dict(A, radius=0), dict(A, strength=0.0)):              # no occlusion: relight with cast shadows
            assert np.array_equal(lighting(orig, depth, L, S, A0), relight_shadowed(orig, depth, L, S)), (L, A0)
            for S0 in (dict(S, maxSteps=0), dict(S, strength=0.0)):        # neither: relight
                assert np.array_equal(lighting(orig, depth, L, S0, A0), relight(orig, depth, L)), (L, S0, A0)


@pytest.mark.parametrize("shape", [(23, 131), (9, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_terms_show(shape):
    """Two-dimensional shapes: on a single row a diagonal march leaves the image at its first step and casts no shadow."""
    rows, cols = shape
    orig, depth = _inputs(rows, cols, 5 + rows)
    common = dict(relief=2.0, ambient=0.75, diffuse=1.5)
    S, A = shadow(64, softness=0.5), occlusion(SHADE, 8, 16, 2.0, 0.0, 1.0)
    for L in (light(DIRECTIONAL, -1, -1, 1, **common), light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common)):
        full = lighting(orig, depth, L, S, A)
        from_shadowed = float((full != relight_shadowed(orig, depth, L, S)).any(-1).mean())
        from_occluded = float((full != occluded(orig, depth, A, L)).any(-1).mean())
        print(f"{shape} kind {L['kind']}: {from_shadowed:.3f} of the pixels differ from relight_shadowed's, {from_occluded:.3f} from the occluded relight's")
        assert from_shadowed > 0.5 and from_occluded > 0.1


def test_the_call_is_declared_named_and_exported():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert re.search(r"\bint rtdd_simulate_lighting\(rtdd_ctx \*ctx,", header)
    assert "rtdd_simulate_lighting" in rt.C_ABI_SYMBOLS and hasattr(rt.Context, "simulate_lighting")
    so = rt.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert re.search(r" T rtdd_simulate_lighting$", out, re.M)
