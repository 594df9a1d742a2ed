"""The aimed depth effects' restatements (tests/refocus_ref.py) pinned on the CPU: refocus against a literal per-pixel gather and
against the oracle's defocus on |d - f|; haze with density and airlight against the oracle's haze at the reference's constants; and
the C ABI declares and the Python mirror names both calls."""
import os
import re

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from effects_ref import effect_inputs
from refocus_ref import (focus_distance, haze_ex, kernel_size, largest_aperture, refocus_by_summed_area_table, refocus_literal,
                         round_f32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_size_is_the_references_at_the_default_aperture():
    for rows, cols, K in ((1080, 1920, 55), (2160, 3840, 110), (4320, 7680, 220)):
        assert kernel_size(rows, cols, 0.025) == K
        assert kernel_size(rows, cols, largest_aperture(rows, cols)) == 255


@pytest.mark.parametrize("shape", [(7, 9), (23, 37), (31, 18)])
@pytest.mark.parametrize("f", [0.0, 37.5, 128.0, 255.0])
def test_summed_area_table_restatement_equals_the_literal_gather(shape, f):
    rows, cols = shape
    orig, depth = effect_inputs(rows, cols, 3 + rows)
    for aperture in (0.0, 0.01, 0.025, 0.4, largest_aperture(rows, cols)):
        want = refocus_literal(orig, depth, f, aperture)
        assert np.array_equal(refocus_by_summed_area_table(orig, depth, f, aperture), want), (f, aperture)


@pytest.mark.parametrize("f", [0.0, 37.5, 128.0, 255.0])
def test_restatement_is_the_oracles_defocus_of_the_focus_distance(oracle, f):
    rows, cols = 67, 121
    orig, depth = effect_inputs(rows, cols, 5)
    want = oracle.defocus(orig, focus_distance(depth, f))
    assert np.array_equal(refocus_by_summed_area_table(orig, depth, f), want)


def test_focus_zero_is_the_defocus_on_a_depth_map(oracle):
    rows, cols = 45, 77
    orig, _ = effect_inputs(rows, cols, 8)
    depth = np.random.default_rng(2).uniform(0, 255, (rows, cols)).astype(np.float32)
    assert np.array_equal(refocus_by_summed_area_table(orig, depth, 0.0), oracle.defocus(orig, depth))


def test_round_f32_is_one_ieee_rounding():
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 1, 2000).astype(np.float32); b = rng.integers(0, 256, 2000).astype(np.float32)
    for x, y in zip(a, b):               # an f32 product is exact in f64: numpy's own rounding of it is the reference
        from fractions import Fraction
        assert round_f32(Fraction(float(x)) * Fraction(float(y))) == Fraction(float(np.float32(np.float64(x) * np.float64(y))))


@pytest.mark.parametrize("contract", [1, 0])
def test_haze_restatement_at_the_references_constants_is_the_oracles_haze(oracle, contract):
    rows, cols = 19, 33
    orig, depth = effect_inputs(rows, cols, 12)
    assert np.array_equal(haze_ex(orig, depth, 2.0, (255, 255, 255), contract, oracle.expf_det), oracle.haze(orig, depth, contract))


def test_header_declares_and_the_mirror_names_the_new_calls():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int rtdd_simulate_refocus\(rtdd_ctx \*ctx,[^;]*double aperture, float focusDepth, int focusX, int focusY\);", code)
    assert re.search(r"int rtdd_simulate_haze_ex\(rtdd_ctx \*ctx,[^;]*float beta, uint8_t airB, uint8_t airG, uint8_t airR\);", code)
    assert {"rtdd_simulate_refocus", "rtdd_simulate_haze_ex"} <= set(rt.C_ABI_SYMBOLS)
    assert hasattr(rt.Context, "simulate_refocus") and hasattr(rt.Context, "simulate_haze_ex")
