"""The restatements of tests/mask_distance_ref.py against each other and against the properties include/rtdd.h states for
rtdd_mask_distance, rtdd_refine_mask and rtdd_lift_layer_matte -- no GPU: the three routes to E agree on every shape and mask the GPU
tests use (tests/mask_distance_cases.py, the border pixels at every reach included); a single pixel's finite distances
are exactly the disc; GROW by 2 is the Chebyshev ring of 1; the feather is monotone in E and saturates exactly where the derived reach
says FAR; the matte lift composited back gives the original; and why the call exists, as two numbers."""
import numpy as np
import pytest

import mask_distance_ref as mr
from mask_distance_cases import EDGE_REACHES, MASKS, SELECTS, SHAPES, make_mask
from composite_ref import NEAREST, composite, layer
from remove_ref import CODE, OTHER, _dilate, lift, mask_pattern

BRUTE_PIXELS = 250                                                          # the brute force walks every pair of pixels: the small shapes
LOHI = [-1023.5, -7.25, -1.0, -0.5, 0.0, 0.5, 1.0, 7.25, 1023.5]


def masks(rows, cols):
    """Every mask of the GPU tests on this shape that does not depend on a reach, by name."""
    return {name: make_mask(name, rows, cols, 0) for name in MASKS if name != "edges"}


# Every shape and mask tests/test_gpu_mask_distance.py compares the kernels with e_scipy on -- "edges" at every reach it is built at --
# under both selects.  A shape above 20000 pixels is split into one test id per mask, and its "edges" per reach.
ROUTE_CASES = [(r, c, None, None) for r, c in SHAPES if r * c <= 20000]
ROUTE_CASES += [(r, c, m, None) for r, c in SHAPES if r * c > 20000 for m in MASKS if m != "edges"]
ROUTE_CASES += [(r, c, "edges", k) for r, c in SHAPES if r * c > 20000 for k in EDGE_REACHES]


@pytest.mark.parametrize("rows,cols,only,reach", ROUTE_CASES, ids=lambda v: str(v))
def test_three_routes_agree(rows, cols, only, reach):
    todo = [(m, k) for m in MASKS for k in (EDGE_REACHES if m == "edges" else [0]) if only is None or (m == only and (reach is None or k == reach))]
    assert todo
    for name, k in todo:
        m = make_mask(name, rows, cols, k)
        for select in SELECTS:
            sel = mr.selected(m, select)
            a, b = mr.e_scipy(sel), mr.e_separable(sel)
            assert np.array_equal(a, b), (name, k, select)
            if rows * cols <= BRUTE_PIXELS:
                assert np.array_equal(mr.e_brute(sel), a), (name, k, select)
            assert (a >= 1).all() and ((a >= mr.INF) == (sel.all() or not sel.any())).all()


def test_the_shapes_are_the_geometry_s():
    from mask_distance_cases import B, H, L, W
    for shape in ((1, 1), (1, 7), (9, 1), (37, 53), (H, W), (H + 1, W + 1), (B, 70), (2 * B + 1, 70), (9, W + 2 * L + 1), (257, 513)):
        assert shape in SHAPES
    assert {1, 2, 5, 63, 64, 65, L, L + 1, 1024} <= set(EDGE_REACHES) and sum(r * c <= BRUTE_PIXELS for r, c in SHAPES) >= 3


@pytest.mark.parametrize("reach", [1, 2, 5, 13])
def test_a_single_pixel_gives_the_disc(reach):
    n = 2 * reach + 5
    m = mr.single_pixels(n, n, [(n // 2, n // 2)])
    sel = mr.selected(m, 0)
    d = mr.distance(mr.e_separable(sel), sel, reach)
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    r2 = yy * yy + xx * xx
    assert d[n // 2, n // 2] == -1 and (d != 0).all()
    outside = r2 > 0
    assert np.array_equal(d[outside & (r2 <= reach * reach)], r2[outside & (r2 <= reach * reach)])
    assert (d[r2 > reach * reach] == mr.FAR).all()
    assert d[n // 2 - reach, n // 2 - reach] == mr.FAR and d[n // 2 + reach, n // 2] == reach * reach      # the box's corner, the disc's pole


def test_grow_by_two_is_the_chebyshev_ring_of_one():
    for name, m in masks(37, 53).items():
        sel = mr.selected(m, CODE)
        got = mr.refine_mask(mr.e_scipy(sel), sel, mr.refine(CODE, mr.GROW, outer2=2))
        assert np.array_equal(got != 0, _dilate(sel, 1)), name


def test_feather_is_monotone_in_e():
    E = np.concatenate([np.arange(1, 5000, dtype=np.int64), np.arange(5000, 1 << 21, 997, dtype=np.int64), [mr.INF]])
    for lo in LOHI:
        for hi in LOHI:
            if lo < hi:
                inside = mr.feather_byte(E, np.ones(E.shape, bool), lo, hi).astype(int)
                outside = mr.feather_byte(E, np.zeros(E.shape, bool), lo, hi).astype(int)
                assert (np.diff(inside) >= 0).all() and (np.diff(outside) <= 0).all(), (lo, hi)
                assert inside[-1] == 255 and outside[-1] == 0


def test_feather_saturates_where_the_derived_reach_says_far():
    """Beyond the reach the host derives, the true E gives exactly the byte a FAR pixel is given: 255 inside, 0 outside."""
    for lo in LOHI:
        for hi in LOHI:
            if lo < hi:
                R = mr.reach_of(mr.refine(0, mr.FEATHER, lo=lo, hi=hi))
                assert 1 <= R <= 1024 and R >= max(abs(lo), abs(hi)) + 0.5 > R - 1
                E = np.concatenate([np.arange(R * R + 1, R * R + 4000, dtype=np.int64), [np.int64(1) << 21, np.int64(1) << 30]])
                assert (mr.feather_byte(E, np.ones(E.shape, bool), lo, hi) == 255).all(), (lo, hi)
                assert (mr.feather_byte(E, np.zeros(E.shape, bool), lo, hi) == 0).all(), (lo, hi)
    for op, kw, want in ((mr.GROW, dict(outer2=1), 1), (mr.GROW, dict(outer2=2), 2), (mr.SHRINK, dict(inner2=25), 5), (mr.SHRINK, dict(inner2=26), 6),
                         (mr.OUTLINE, dict(inner2=4096, outer2=4097), 65), (mr.OUTLINE, dict(inner2=1024 * 1024), 1024)):
        assert mr.reach_of(mr.refine(0, op, **kw)) == want


def test_distance_and_refine_agree_at_the_derived_reach():
    m = mask_pattern("disc", 61, 83); m[3, 70] = OTHER
    for select in (0, CODE):
        sel = mr.selected(m, select)
        E = mr.e_scipy(sel)
        for R in (mr.refine(select, mr.GROW, outer2=26), mr.refine(select, mr.SHRINK, inner2=24), mr.refine(select, mr.OUTLINE, inner2=1, outer2=16),
                  mr.refine(select, mr.OUTLINE, outer2=2), mr.refine(select, mr.FEATHER, lo=-7.25, hi=0.5), mr.refine(select, mr.FEATHER, lo=-1.0, hi=1.0)):
            assert np.array_equal(mr.refine_from_distance(mr.distance(E, sel, mr.reach_of(R)), R), mr.refine_mask(E, sel, R)), R


def test_matte_lift_composited_back_gives_the_original():
    rows, cols = 41, 57
    rng = np.random.default_rng(5)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    alpha = rng.integers(0, 256, (rows, cols), dtype=np.uint8); alpha[rng.random((rows, cols)) < 0.3] = 0; alpha[rng.random((rows, cols)) < 0.3] = 255
    for x, y, sr, sc in ((0, 0, rows, cols), (-5, 7, 30, 40), (20, -3, 60, 60)):
        sprite = mr.lift_matte(orig, alpha, x, y, sr, sc)
        assert np.array_equal(composite(orig, depth, sprite, layer(sr, sc, x, y, 256, NEAREST, 255))[0], orig)
    hard = np.where(alpha >= 128, 255, 0).astype(np.uint8)
    assert np.array_equal(mr.lift_matte(orig, hard, -5, 7, 30, 40), lift(orig, hard, 0, -5, 7, 30, 40))


def outline_step(feather):
    """A gray disc with an anti-aliased edge on a white wall, selected as a wand selects it (every pixel the disc touches), is moved onto
    a black wall: the mean absolute step between the pixels just inside and just outside the moved selection's outline."""
    n, r, move = 96, 20.0, 40
    yy, xx = np.mgrid[0:n, 0:2 * n]
    cover = np.clip(r + 0.5 - np.sqrt((yy - n / 2) ** 2 + (xx - n / 2) ** 2), 0, 1)           # the disc's share of each pixel
    orig = np.repeat((255 - cover * 127 + 0.5).astype(np.uint8)[..., None], 3, 2)
    sel = cover > 0
    E = mr.e_scipy(sel)
    alpha = mr.refine_mask(E, sel, mr.refine(0, mr.FEATHER, lo=-feather, hi=0.0)) if feather else np.where(sel, 255, 0).astype(np.uint8)
    sprite = mr.lift_matte(orig, alpha, 0, 0, n, 2 * n)
    black = np.zeros_like(orig)
    out = composite(black, np.zeros((n, 2 * n), np.float32), sprite, layer(n, 2 * n, move, 0, 256, NEAREST, 255))[0].astype(int)
    moved = np.zeros_like(sel); moved[:, move:] = sel[:, :-move]
    steps = []
    for dy, dx in ((0, 1), (1, 0)):
        a, b = moved[:n - dy, :2 * n - dx], moved[dy:, dx:]
        pa, pb = out[:n - dy, :2 * n - dx], out[dy:, dx:]
        steps.append(np.abs(pa - pb)[a != b].ravel())
    return float(np.concatenate(steps).mean())


def test_why_the_call_exists(capsys):
    hard, soft = outline_step(0.0), outline_step(3.0)
    with capsys.disabled():
        print(f"\nmean absolute step across a moved disc's outline: hard lift {hard:.1f}, --move-feather 3 {soft:.1f}")
    assert soft < hard
