"""The depth regions without a GPU: the restatement (tests/regions_ref.py) against the maps it must reduce to and against a second,
per-pixel restatement of the rule; the two cases that motivate the feature, solved with the numpy restatement of the solver -- a weak edge
that leaks and a texture that blocks; and the declarations of the interface (include/rtdd.h, the Python wrapper).

The two scenes assert comparisons only and print the errors they compare (pytest -s)."""
import os
import re

import numpy as np
import pytest

import np_restatement as npr
import realtimedepthdiffusion_amd as rt
import regions_ref as rr
from color_guide_ref import BGR, GRAY, index_maps_bgr, isoluminant_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = [(2, 2), (1, 2), (0, 2)]              # (level, maxLevel): un-gated; gated with threshold 4; gated with threshold 0


def _random_case(seed, rows=23, cols=31):
    rng = np.random.default_rng(seed)
    gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(90, 120, (rows, cols)).astype(np.float32)
    depth[:, ::3] = np.floor(depth[:, ::3] / 3) * 3             # neighbouring differences on both sides of both thresholds
    codes = rng.integers(0, 3, (rows, cols)).astype(np.uint8)   # 0 (unassigned), 1, 2: equal and different neighbours of every kind
    return gray, bgr, depth, codes


def test_all_zero_codes_and_flags_0_give_the_base_maps():
    gray, bgr, depth, codes = _random_case(1)
    for level, max_level in REGIMES:
        for base in (npr.index_maps(gray, depth, level, max_level), index_maps_bgr(bgr, depth, level, max_level)):
            for flags in (0, rr.CUT, rr.SMOOTH, rr.CUT | rr.SMOOTH):
                zero = rr.index_maps_regions(base, np.zeros_like(codes), flags)
                off = rr.index_maps_regions(base, codes, 0)
                for k in base:
                    assert np.array_equal(zero[k], base[k]) and np.array_equal(off[k], base[k]), (level, max_level, flags, k)


def _rule_by_loops(maps, codes, flags):
    """The rule once more, pixel by pixel and neighbour by neighbour, as include/rtdd.h states it."""
    rows, cols = codes.shape
    out = {k: v.copy() for k, v in maps.items()}
    for y in range(rows):
        for x in range(cols):
            for k, (dx, dy) in (("left", (-1, 0)), ("right", (1, 0)), ("up", (0, -1)), ("down", (0, 1))):
                nx, ny = x + dx, y + dy
                if nx < 0 or ny < 0 or nx >= cols or ny >= rows:
                    assert maps[k][y, x] == 256
                    continue
                rp, rq = int(codes[y, x]), int(codes[ny, nx])
                if flags & rr.CUT and rp != rq:
                    out[k][y, x] = 255
                elif flags & rr.SMOOTH and rp == rq and rp != 0:
                    out[k][y, x] = 0
    return out


@pytest.mark.parametrize("regime", REGIMES, ids=lambda r: f"{r[0]}of{r[1]}")
def test_the_array_restatement_is_the_rule_pixel_by_pixel(regime):
    level, max_level = regime
    gray, bgr, depth, codes = _random_case(2 + level)
    for base in (npr.index_maps(gray, depth, level, max_level), index_maps_bgr(bgr, depth, level, max_level)):
        for flags in (rr.CUT, rr.SMOOTH, rr.CUT | rr.SMOOTH):
            got, want = rr.index_maps_regions(base, codes, flags), _rule_by_loops(base, codes, flags)
            for k in base:
                assert np.array_equal(got[k], want[k]), (regime, flags, k)
            inner = got["right"][:, :-1]
            if flags & rr.CUT:
                assert (inner == 255).any()
            if flags & rr.SMOOTH:
                assert ((inner == 0) & (base["right"][:, :-1] != 0)).any()
            assert ((inner == base["right"][:, :-1]) & (inner != 0) & (inner != 255)).any()       # ... and some edges are left alone
            assert (got["right"][:, -1] == 256).all() and (got["up"][0] == 256).all()


def _pair_problem(rows=24, cols=40):
    """The colour guide's example (tests/test_color_guide_cpu.py): split down the middle between two colours of one luminance, labels 0
    and 255 on the two outer columns, the start depth constant in between."""
    bgr = isoluminant_image(rows, cols)
    mask = np.zeros((rows, cols), np.uint8)
    mask[:, 0] = 255; mask[:, -1] = 255
    depth = np.full((rows, cols), 128.0, np.float32)
    depth[:, 0] = 0.0; depth[:, -1] = 255.0
    return bgr, mask, depth


def test_the_cut_survives_the_gate(oracle, lut):
    """Level 0 of 1, the start depth constant across the boundary: the gate zeroes every edge there before either guide is asked, so
    neither guide can hold the boundary; codes 1 | 2 with CUT do -- the override comes after the gate."""
    bgr, mask, depth = _pair_problem()
    rows, cols = mask.shape
    b = cols // 2
    gray = oracle.bgr2gray(bgr)
    codes = np.ones((rows, cols), np.uint8); codes[:, b:] = 2
    for kind, guide in ((GRAY, gray), (BGR, bgr)):
        base = rr.base_maps(guide, kind, depth, 0, 1)
        assert (base["right"][:, b - 1] == 0).all() and (base["left"][:, b] == 0).all()        # hidden from both guides
        cut = rr.index_maps_regions(base, codes, rr.CUT)
        assert (cut["right"][:, b - 1] == 255).all() and (cut["left"][:, b] == 255).all()
        changed = cut["right"] != base["right"]
        assert changed[:, b - 1].all() and changed.sum() == rows                                 # the boundary edges and no other
        assert np.array_equal(cut["up"], base["up"]) and np.array_equal(cut["down"], base["down"])
        x = rr.solve_regions(depth, mask, guide, kind, codes, rr.CUT, 300, 0, 1, lut, 1)
        plain = rr.solve_regions(depth, mask, guide, kind, codes, 0, 300, 0, 1, lut, 1)
        jump, plain_jump = float(np.abs(x[:, b] - x[:, b - 1]).min()), float(np.abs(plain[:, b] - plain[:, b - 1]).min())
        print(f"guide {kind}: jump across the boundary after 300 sweeps {jump:.4g} with the cut, {plain_jump:.4g} without")
        assert jump > plain_jump


# ---- a weak edge leaks -------------------------------------------------------------------------------------------------------------------
def _ellipse_scene(step, seed=5):
    """tests/test_fill_similar_cpu.py's scene: a 48 x 40 image, an ellipse of 513 pixels of gray 100 on gray 100 + step, noise in [-2, 2]."""
    rows, cols = 48, 40
    yy, xx = np.mgrid[:rows, :cols]
    obj = ((yy - 24) / 15) ** 2 + ((xx - 20) / 11) ** 2 <= 1
    assert obj.sum() == 513
    gray = (np.where(obj, 100, 100 + step) + np.random.default_rng(seed).integers(-2, 3, (rows, cols))).astype(np.uint8)
    return obj, gray


def test_a_cut_region_holds_a_weak_edge(lut):
    """The wand's documented limit: a step of 8 gray levels under noise of +-2 is no boundary, for the wand or for the solver.  Truth 200 on
    the ellipse and 40 around it, one 5 x 5 stamp of each label, level 0 of 0.  Without regions the labels leak into each other and the
    error does not recover with more sweeps; with the ellipse as region 1 and RTDD_REGION_CUT it falls towards 0.  Asserted where a single
    level has had the sweeps to cover a 48 x 40 image (1000, 3000): the error with the cut is below half of the error without.  300 sweeps
    are printed only -- what is left there is single-level convergence, which the cascade exists for."""
    obj, gray = _ellipse_scene(8)
    rows, cols = gray.shape
    truth = np.where(obj, 200.0, 40.0)
    e, s = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
    for (x, y), label in (((20, 24), 200), ((3, 3), 40)):
        e[y - 2:y + 3, x - 2:x + 3] = label; s[y - 2:y + 3, x - 2:x + 3] = 255
    depth = np.where(s == 255, e, 128).astype(np.float32)
    codes = obj.astype(np.uint8)
    for sweeps in (300, 1000, 3000):
        without = float(np.abs(rr.solve_regions(depth, s, gray, GRAY, codes, 0, sweeps, 0, 0, lut, 1) - truth).mean())
        with_cut = float(np.abs(rr.solve_regions(depth, s, gray, GRAY, codes, rr.CUT, sweeps, 0, 0, lut, 1) - truth).mean())
        print(f"mean |depth - truth| after {sweeps} sweeps: without regions {without:.1f}, the ellipse cut {with_cut:.2f}")
        if sweeps >= 1000:
            assert with_cut < 0.5 * without


# ---- a texture blocks ----------------------------------------------------------------------------------------------------------------------
def _floor_scene(seed=7):
    """56 x 48: a wall of gray 255 around a floor of random 4 x 4 tiles of gray 0..127 -- a corridor 40 rows long and 24 pixels wide whose
    borders are tile borders, so every floor pixel has a neighbour of its own gray.  The floor's true depth is a plane, 60 at its far
    edge to 220 at the near one; the annotation is one 3-pixel ramp stroke down its middle, and a stamp on the wall.  The step between wall
    and floor is at least 128 gray levels, a weight below 6e-23: the wall cannot leak into the floor with or without a cut.  (Longer than
    wide: a plane is harmonic and fits the cut sides, but not the cut ends, so the smoothed solution leaves it within about a width of
    the two ends.)"""
    rows, cols, top = 56, 48, 16
    yy, xx = np.mgrid[:rows, :cols]
    floor = (yy >= top) & (xx >= 12) & (xx < 36)
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 128, (rows // 4, cols // 4)).astype(np.uint8)
    gray = np.where(floor, np.repeat(np.repeat(tiles, 4, 0), 4, 1), 255).astype(np.uint8)
    plane = 60.0 + (yy - top) * (160.0 / (rows - 1 - top))
    s = np.zeros((rows, cols), np.uint8)
    depth = np.full((rows, cols), 128.0, np.float32)
    s[top:, 23:26] = 255; depth[top:, 23:26] = np.floor(plane[top:, 23:26] + 0.5)
    s[3:8, 5:10] = 255; depth[3:8, 5:10] = 30.0
    return floor, gray, plane, s, depth


def test_a_smoothed_region_crosses_a_texture(lut):
    """The lasso's motivating case: the tiles' edges stop the diffusion inside one surface, and the only cure so far is to label every
    pixel of it.  With the floor as region 1: the cut alone is no better than nothing (the wall does not leak in either way, and the
    tiles block as before); cut and smooth together are below half of the error without regions, and below half of the cut's."""
    floor, gray, plane, s, depth = _floor_scene()
    codes = floor.astype(np.uint8)
    print(f"the floor has {int(floor.sum())} pixels")
    for sweeps in (300, 1000):
        err = {}
        for name, flags in (("none", 0), ("cut", rr.CUT), ("cut+smooth", rr.CUT | rr.SMOOTH)):
            x = rr.solve_regions(depth, s, gray, GRAY, codes, flags, sweeps, 0, 0, lut, 1)
            err[name] = float(np.abs(x - plane)[floor].mean())
        print(f"mean |depth - plane| on the floor after {sweeps} sweeps: " + ", ".join(f"{k} {v:.6f}" for k, v in err.items()))
        assert err["cut"] >= err["none"]
        assert err["cut+smooth"] < 0.5 * err["none"] and err["cut+smooth"] < 0.5 * err["cut"]


# ---- the code planes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (45, 61), (181, 243)])
def test_region_codes_sample_the_top_left_pixel(rows, cols):
    rng = np.random.default_rng(rows)
    edited = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    mask = np.where(rng.random((rows, cols)) < 0.6, 255, rng.integers(0, 255, (rows, cols))).astype(np.uint8)
    for level in range(4):
        got = rr.region_codes(edited, mask, level)
        r, c = rows >> level, cols >> level
        assert got.shape == (r, c) == (int(np.float32(rows) / np.float32(2.0) ** level), int(np.float32(cols) / np.float32(2.0) ** level))
        for y in range(r):
            for x in range(c):
                sy, sx = y << level, x << level
                assert sy < rows and sx < cols                                  # the sample always lies inside level 0
                assert got[y, x] == (edited[sy, sx, 0] if mask[sy, sx] == 255 else 0)
    # top-left sampling composes: level 2 of the pair is level 1 of level 1's codes
    if rows >= 4 and cols >= 4:
        l1 = rr.region_codes(edited, mask, 1)
        assert np.array_equal(rr.region_codes(edited, mask, 2), l1[::2, ::2][:rows >> 2, :cols >> 2])


# ---- the interface: these fail without the feature, with or without a GPU ----------------------------------------------------------------
NEW_FUNCTIONS = ["rtdd_solve_regions", "rtdd_index_to_weight_regions", "rtdd_region_codes", "rtdd_pyramid_set_regions", "rtdd_pyramid_regions",
                 "rtdd_pyramid_regions_changed"]


def _header():
    text = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_region_interface():
    text, code = _header()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(\s*rtdd_ctx\s*\*" % name, code), name
    assert re.search(r"enum\s+rtdd_region_flags\s*\{\s*RTDD_REGION_CUT\s*=\s*1\s*,\s*RTDD_REGION_SMOOTH\s*=\s*2\s*\}", code)
    for name, value in (("RTDD_IMG_REGION_EDITED", 8), ("RTDD_IMG_REGION_MASK", 9), ("RTDD_IMG_REGION_CODE", 10)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), code), name
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for words in ("THE OVERRIDE COMES AFTER THE GATE", "the index stays 256", "LUT[255], not 0", "denormal divisor", "IS rtdd_solve_guided"):
        assert words in flat, words
    assert re.search(r"next bump of RTDD_VERSION should cover them", flat[flat.index("Depth regions"):flat.index("enum rtdd_region_flags")])


def test_version_is_unchanged():
    text, _ = _header()
    assert re.search(r"#define\s+RTDD_VERSION\s+230\b", text)


def test_wrapper_exposes_the_region_interface():
    assert (rt.REGION_CUT, rt.REGION_SMOOTH) == (1, 2) == (rr.CUT, rr.SMOOTH)
    assert (rt.IMG_REGION_EDITED, rt.IMG_REGION_MASK, rt.IMG_REGION_CODE) == (8, 9, 10)
    for name in NEW_FUNCTIONS:
        assert name in rt.C_ABI_SYMBOLS, name
    for method in ("solve_regions", "index_to_weight_regions", "region_codes", "pyramid_set_regions", "pyramid_regions", "pyramid_regions_changed"):
        assert callable(getattr(rt.Context, method, None)), method
