"""The occlusion-aware lens blur's definition (include/rtdd.h rtdd_simulate_bokeh) on the CPU: the two restatements of tests/bokeh_ref.py
agree, the header's three identities hold, the two-layer scene shows what the effect is for, and the header's constants are right."""
import numpy as np
import pytest

from bokeh_ref import (bokeh_by_offsets, bokeh_by_offsets_s, bokeh_literal, signed_coc, two_layer_scene, weights)
from effect_gpu import random_inputs
from lens_blur_ref import disc_diameter, disc_points, lens_blur_by_row_prefixes_k
from refocus_ref import focus_distance


@pytest.mark.parametrize("K,f", [(127, 100.0), (9, 100.0), (127, 300.0)])
def test_the_two_restatements_agree(K, f):
    orig, depth = random_inputs(23, 31, 7)
    assert np.isnan(depth).any() and (depth < 0).any() and (depth > 255).any()
    got = bokeh_by_offsets(orig, depth, f, K)
    assert np.array_equal(got, bokeh_literal(orig, depth, f, K))
    assert not np.array_equal(got, orig)
    # a band of output rows is those rows of the whole
    assert np.array_equal(bokeh_by_offsets(orig, depth, f, K, band=(5, 17)), got[5:17])


def test_signed_circle_is_the_discs_diameter_inside_the_range():
    depth = np.random.default_rng(3).uniform(0, 255, (40, 50)).astype(np.float32)
    for K in (0, 1, 55, 127):
        for f in (0.0, 37.5, 255.0):
            s = signed_coc(depth, f, K)
            assert np.array_equal(np.abs(s), disc_diameter(K, focus_distance(depth, f)))
            assert (np.abs(s) <= K).all() and ((s < 0) == ((depth < np.float32(f)) & (s != 0))).all()
    s = signed_coc(np.array([[np.nan, -5.0, 300.0, 100.0]], np.float32), np.nan, 127)       # a NaN focus is 0, as a NaN depth
    assert s.tolist() == [[0, 0, 127, 49]]


@pytest.mark.parametrize("k", [0, 1, 2, 3, 9, 40, 127])
def test_constant_circle_is_the_disc_gather(k):
    orig = random_inputs(45, 70, 11)[0]
    for sign in (1, -1):
        s = np.full(orig.shape[:2], sign * k, np.int64)
        assert np.array_equal(bokeh_by_offsets_s(orig, s)[0], lens_blur_by_row_prefixes_k(orig, np.abs(s)))


def test_circles_of_at_most_one_give_the_original():
    orig = random_inputs(30, 41, 12)[0]
    s = np.random.default_rng(5).integers(-1, 2, orig.shape[:2])
    assert np.array_equal(bokeh_by_offsets_s(orig, s)[0], orig)


def test_a_pixel_in_focus_with_nothing_in_front_keeps_its_bytes():
    orig = random_inputs(40, 52, 13)[0]
    s = np.random.default_rng(6).integers(0, 60, orig.shape[:2])
    s[np.random.default_rng(7).random(s.shape) < 0.3] = 0
    out = bokeh_by_offsets_s(orig, s)[0]
    assert np.array_equal(out[s == 0], orig[s == 0]) and not np.array_equal(out[s > 1], orig[s > 1])
    s[3, 4] = -50                                                     # ... and one pixel in front spills onto the sharp ones near it
    out = bokeh_by_offsets_s(orig, s)[0]
    assert not np.array_equal(out[s == 0], orig[s == 0])


def test_two_layer_scene():
    orig, depth, sq, K = two_layer_scene()
    # focus on the square: it stays as it is and nothing of it leaks into the blurred background -- the disc gather has a red halo
    out = bokeh_by_offsets(orig, depth, 10.0, K)
    assert np.array_equal(out[sq], orig[sq])
    assert (out[~sq][:, 2] == 0).all()
    disc = lens_blur_by_row_prefixes_k(orig, disc_diameter(K, focus_distance(depth, 10.0)))
    assert np.array_equal(disc[sq], orig[sq])
    assert int((disc[~sq][:, 2] > 0).sum()) == 2228 and int(disc[~sq][:, 2].max()) == 121
    # focus on the background: the blurred square spills softly over it -- the disc gather keeps a hard silhouette
    out = bokeh_by_offsets(orig, depth, 200.0, K)
    assert int((out[~sq][:, 2] > 0).sum()) == 2228
    disc = lens_blur_by_row_prefixes_k(orig, disc_diameter(K, focus_distance(depth, 200.0)))
    assert (disc[~sq][:, 2] == 0).all()


def test_the_headers_constants():
    wt = weights()
    assert disc_points(0) == 1 and disc_points(1) == 1 and disc_points(127) == 12645
    assert wt[127] == 84914 and wt[0] == wt[1] == 1 << 30 and (np.diff(wt) <= 0).all() and len(wt) == 128
    orig, depth = random_inputs(23, 31, 7)
    smax = max(bokeh_by_offsets_s(orig, signed_coc(depth, 100.0, K))[1] for K in (127, 9))
    print(f"largest S_c on the random case: 2^{np.log2(smax):.1f}")
    assert 0 < smax < 1 << 52
