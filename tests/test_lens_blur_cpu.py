"""The round-aperture lens blur without a GPU: the three restatements of tests/lens_blur_ref.py against each other, the facts the
kernels' exactness rests on (point counts, count < 2^16, sums < 2^24), and the new entry point in both built libraries."""
import os
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from lens_blur_ref import (disc_diameter, disc_points, lens_blur_by_row_prefixes, lens_blur_by_row_prefixes_k, lens_blur_constant_k,
                           lens_blur_literal, lens_blur_literal_k)
from refocus_ref import kernel_size, largest_aperture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "realtimedepthdiffusion_amd")


def _image(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


@pytest.mark.parametrize("rows,cols", [(60, 80), (23, 37), (1, 50), (50, 1), (1, 1), (9, 300)])
def test_literal_gather_equals_row_prefixes_on_random_maps(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    orig = _image(rows, cols, 1)
    depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    for aperture, f in ((0.025, 0.0), (0.2, 100.0), (largest_aperture(rows, cols), 37.5)):
        assert np.array_equal(lens_blur_literal(orig, depth, f, aperture), lens_blur_by_row_prefixes(orig, depth, f, aperture)), (aperture, f)


def test_literal_gather_equals_row_prefixes_for_the_named_diameters():
    """k = 0, 1, 2, 102, 103 and 255 (and their neighbours), with windows clipped at every border: the image is smaller than the
    largest disc, so every large window is clipped on all four sides somewhere."""
    rows, cols = 40, 56
    orig = _image(rows, cols, 2)
    rng = np.random.default_rng(3)
    k = rng.choice(np.array([0, 1, 2, 3, 4, 5, 101, 102, 103, 104, 254, 255]), (rows, cols))
    k[0, 0] = k[0, -1] = k[-1, 0] = k[-1, -1] = 255; k[rows // 2, cols // 2] = 255
    k[0, 1] = 103; k[1, 0] = 102; k[-1, 1] = 2; k[1, -1] = 1
    assert np.array_equal(lens_blur_literal_k(orig, k), lens_blur_by_row_prefixes_k(orig, k))
    for band in ((0, 7), (7, 33), (33, 40)):
        assert np.array_equal(lens_blur_by_row_prefixes_k(orig, k, band), lens_blur_by_row_prefixes_k(orig, k)[band[0]:band[1]])


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 17, 56, 57, 102, 103, 255])
def test_row_prefixes_equal_the_correlation_for_a_constant_diameter(k):
    rows, cols = (70, 90) if k < 200 else (96, 110)
    orig = _image(rows, cols, 4 + k)
    assert np.array_equal(lens_blur_by_row_prefixes_k(orig, np.full((rows, cols), k, np.int64)), lens_blur_constant_k(orig, k))


def test_point_counts_and_the_bounds_the_exact_sums_rest_on():
    assert [disc_points(k) for k in range(6)] == [1, 1, 5, 9, 13, 21]
    assert disc_points(255) == 51101
    assert max(disc_points(k) for k in range(256)) == 51101 < 2 ** 16
    assert 51101 * 255 < 2 ** 24
    # the packed 3 x 21-bit accumulator holds a whole disc up to k = 102, and 32 rows of any disc
    assert disc_points(102) == 8173 and disc_points(103) == 8341
    assert 8173 * 255 < 2 ** 21 <= 8341 * 255
    assert 32 * 255 * 255 < 2 ** 21
    # the counts by spans are the counts by points
    for k in (0, 1, 2, 3, 57, 102, 103, 254, 255):
        n = sum(2 * int(np.sqrt((k * k - 4 * dy * dy) // 4 + 0.5)) + 1 for dy in range(-(k // 2), k // 2 + 1))
        assert n == disc_points(k), k


def test_the_diameter_is_clamped_and_total():
    d = np.array([0.0, 1.0, 254.9, 255.0, 300.0, 1e9, -7.5, np.nan, np.inf, -np.inf], np.float32)
    assert disc_diameter(255, d).tolist() == [0, 1, 254, 255, 255, 255, 0, 0, 255, 0]
    assert disc_diameter(0, d).tolist() == [0] * 10
    assert disc_diameter(55, np.abs(d)).tolist() == [0, 0, 54, 55, 64, 255, 1, 0, 255, 255]
    # f32 product, double quotient, truncation -- and (int)(v / 255) is the floor of the exact quotient for every f32 product v
    v = np.random.default_rng(5).uniform(0, 65025, 200000).astype(np.float32)
    assert np.array_equal(disc_diameter(1, v), np.floor(v.astype(np.float64) / 255.0).astype(np.int64))


def test_small_diameters_and_constant_images_give_the_image():
    rows, cols = 33, 47
    orig = _image(rows, cols, 6)
    for k in (0, 1):
        assert np.array_equal(lens_blur_by_row_prefixes_k(orig, np.full((rows, cols), k, np.int64)), orig)
        assert np.array_equal(lens_blur_literal_k(orig, np.full((rows, cols), k, np.int64)), orig)
    depth = np.random.default_rng(7).uniform(0, 255, (rows, cols)).astype(np.float32)
    assert kernel_size(rows, cols, 0.0) == 0
    assert np.array_equal(lens_blur_by_row_prefixes(orig, depth, 50.0, 0.0), orig)
    flat = np.empty_like(orig); flat[...] = (13, 200, 255)
    for aperture in (0.025, 0.5, largest_aperture(rows, cols)):
        assert np.array_equal(lens_blur_by_row_prefixes(flat, depth, 99.0, aperture), flat)


@pytest.mark.parametrize("lib", ["librtdd.so", "librtdd_acq.so"])
def test_both_libraries_export_the_entry_point(lib):
    path = os.path.join(PKG, lib)
    assert os.path.exists(path), f"{path} is not built"
    names = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    assert " T rtdd_simulate_lens_blur" in names


def test_the_python_interface_has_the_method_and_the_shapes():
    assert callable(getattr(rt.Context, "simulate_lens_blur"))
    assert (rt.APERTURE_BOX, rt.APERTURE_DISC) == (0, 1)
    assert "rtdd_simulate_lens_blur" in rt.C_ABI_SYMBOLS
    with open(os.path.join(ROOT, "include", "rtdd.h")) as f:
        header = f.read()
    assert "RTDD_APERTURE_BOX = 0, RTDD_APERTURE_DISC = 1" in header and "int rtdd_simulate_lens_blur(" in header
