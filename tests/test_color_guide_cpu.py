"""The colour guide without a GPU: its restatement (tests/color_guide_ref.py) against the gray one it must reduce to, the isoluminant
pair that motivates it, and the declarations of the interface (include/rtdd.h, the Python wrapper).

What the gate does to a colour edge (stated in include/rtdd.h): at level 0 of a cascade (gated, threshold 0) an edge whose two pixels
start at the same u8 depth has index 0 under EITHER guide, so both guides give the same result there -- a colour edge has to be found at
the coarsest level, which is not gated, and inherited (test_level_0_gate_hides_the_colour_edge_from_both_guides)."""
import os
import re

import numpy as np

import np_restatement as npr
import realtimedepthdiffusion_amd as rt
from color_guide_ref import GREEN, RED, index_maps_bgr, isoluminant_image, solve_bgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, SWEEPS = 24, 40, 300


def test_replicated_gray_gives_the_gray_indices():
    rng = np.random.default_rng(5)
    gray = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    depth = rng.uniform(-10, 270, gray.shape).astype(np.float32)
    depth[rng.random(gray.shape) < 0.05] = np.nan
    depth[:, ::3] = np.floor(depth[:, ::3] / 3) * 3             # neighbouring differences on both sides of both thresholds
    bgr = np.repeat(gray[..., None], 3, axis=2)
    for level, max_level in ((2, 2), (1, 2), (0, 2)):           # un-gated; gated with threshold 4; gated with threshold 0
        want, got = npr.index_maps(gray, depth, level, max_level), index_maps_bgr(bgr, depth, level, max_level)
        for k in want:
            assert np.array_equal(got[k], want[k]), (level, max_level, k)
    assert not np.array_equal(npr.index_maps(gray, depth, 0, 2)["right"], npr.index_maps(gray, depth, 1, 2)["right"])
    assert not np.array_equal(npr.index_maps(gray, depth, 1, 2)["right"], npr.index_maps(gray, depth, 2, 2)["right"])


def test_the_index_is_the_largest_channel_difference():
    bgr = np.zeros((2, 2, 3), np.uint8)
    bgr[0, 0] = (10, 200, 30); bgr[0, 1] = (250, 190, 30); bgr[1, 0] = (10, 200, 31); bgr[1, 1] = (0, 0, 0)
    m = index_maps_bgr(bgr, np.zeros((2, 2), np.float32), 0, 0)
    assert m["right"][0, 0] == 240 and m["left"][0, 1] == 240 and m["down"][0, 0] == 1 and m["up"][1, 0] == 1
    assert m["right"][1, 0] == 200 and m["down"][0, 1] == 250
    assert m["left"][0, 0] == 256 and m["up"][0, 0] == 256 and m["right"][0, 1] == 256 and m["down"][1, 1] == 256


def _pair_problem():
    """The issue's example: 24 x 40, split down the middle between the two colours, labels 0 and 255 on the two outer columns."""
    bgr = isoluminant_image(ROWS, COLS)
    mask = np.zeros((ROWS, COLS), np.uint8)
    mask[:, 0] = 255; mask[:, -1] = 255
    depth = np.full((ROWS, COLS), 128.0, np.float32)
    depth[:, 0] = 0.0; depth[:, -1] = 255.0
    return bgr, mask, depth


def test_isoluminant_pair_is_invisible_to_gray_and_visible_to_colour(oracle, lut):
    bgr, mask, depth = _pair_problem()
    gray = oracle.bgr2gray(bgr)
    assert int(oracle.bgr2gray(np.array([[GREEN]], np.uint8))[0, 0]) == 59 and int(oracle.bgr2gray(np.array([[RED]], np.uint8))[0, 0]) == 59
    assert (gray == 59).all()
    # at level == maxLevel (no gate) the gray-guided solve cannot tell the image from a constant one
    by_gray = npr.solve(depth, mask, gray, SWEEPS, 0, 0, lut, 1)
    constant = npr.solve(depth, mask, np.full_like(gray, 200), SWEEPS, 0, 0, lut, 1)
    assert np.array_equal(by_gray.view(np.uint32), constant.view(np.uint32))
    by_colour = solve_bgr(depth, mask, bgr, SWEEPS, 0, 0, lut, 1)
    b = COLS // 2

    def jump(x):
        return float(np.abs(x[:, b] - x[:, b - 1]).min())
    print(f"jump across the boundary: gray guide {jump(by_gray):.4g}, colour guide {jump(by_colour):.4g}")
    assert jump(by_colour) > jump(by_gray)                      # a comparison, not a threshold


def test_level_0_gate_hides_the_colour_edge_from_both_guides(oracle, lut):
    """Level 0 of a two-level cascade, initial depth constant across the boundary: the gate zeroes the index of every edge there before
    the guide is asked, so the two guides give the same bits."""
    bgr, mask, depth = _pair_problem()
    gray = oracle.bgr2gray(bgr)
    assert np.array_equal(solve_bgr(depth, mask, bgr, 50, 0, 1, lut, 1).view(np.uint32), npr.solve(depth, mask, gray, 50, 0, 1, lut, 1).view(np.uint32))


# ---- the interface: these fail without the feature, with or without a GPU ----------------------------------------------------------------
NEW_FUNCTIONS = ["rtdd_solve_guided", "rtdd_index_to_weight_guided", "rtdd_pyrdown_bgr", "rtdd_pyramid_set_guide", "rtdd_pyramid_guide"]


def _header():
    text = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_guided_interface():
    _, code = _header()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(\s*rtdd_ctx\s*\*" % name, code), name
    assert re.search(r"enum\s+rtdd_guide\s*\{\s*RTDD_GUIDE_GRAY\s*=\s*0\s*,\s*RTDD_GUIDE_BGR\s*=\s*1\s*\}", code)
    assert re.search(r"RTDD_IMG_GUIDE_BGR\s*=\s*7\b", code)


def test_version_is_unchanged():
    text, _ = _header()
    assert re.search(r"#define\s+RTDD_VERSION\s+230\b", text)


def test_wrapper_exposes_the_guided_interface():
    assert (rt.GUIDE_GRAY, rt.GUIDE_BGR, rt.IMG_GUIDE_BGR) == (0, 1, 7)
    for name in NEW_FUNCTIONS:
        assert name in rt.C_ABI_SYMBOLS, name
    for method in ("solve_guided", "index_to_weight_guided", "pyrdown_bgr", "pyramid_set_guide", "pyramid_guide"):
        assert callable(getattr(rt.Context, method, None)), method
