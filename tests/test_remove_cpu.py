"""rtdd_remove_object and rtdd_lift_layer (include/rtdd.h) without a GPU: the two restatements of tests/remove_ref.py agree on every shape,
mask, grow, select, source limit and wild depth of the issue; the header's identities; the lift / remove / composite identity through
composite_ref.composite; the two measurements that motivated the rule, as inequalities; and the C ABI lists the two entry points."""
import functools

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from composite_ref import NEAREST, composite, layer
from dataset_util import load_pair
from remove_ref import (CODE, OTHER, classes, lift, mask_pattern, nearest_in_row, remove, remove_literal, removal, same_bits, selected)
from roi_util import covering

F = np.float32
SHAPES = [(1, 1), (1, 7), (9, 1), (37, 53), (65, 33)]
MASKS = ["random", "checker", "borders", "all", "none", "allbut"]
GROWS = [0, 1, 3, 8]
SELECTS = [0, CODE]
LIMITS = [0.0, 100.0]


@functools.lru_cache(maxsize=None)
def inputs(rows, cols):
    """A random image and a depth map in [-20, 275] with 3 % NaN and a -0."""
    rng = np.random.default_rng(rows * 100 + cols)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(F)
    depth[rng.random((rows, cols)) < 0.03] = np.nan
    depth[rows // 2, cols // 2] = F(-0.0)
    return orig, depth


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).any(-1).sum())} pixels differ"
    assert same_bits(got[1], want[1]), f"{what}: {int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())} depths differ"


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_two_restatements_agree(rows, cols):
    orig, depth = inputs(rows, cols)
    arity, filled, bystanders, nan_kept = set(), 0, 0, 0
    for mi, gi, si, li in covering(len(MASKS), len(GROWS), len(SELECTS), len(LIMITS)):
        mask = mask_pattern(MASKS[mi], rows, cols, seed=mi + 3)
        R = removal(SELECTS[si], GROWS[gi], LIMITS[li])
        counts = {}
        want = remove(orig, depth, mask, R, counts)
        got = remove_literal(orig, depth, mask, R, arity if MASKS[mi] == "random" else None)
        assert_same(got, want, (rows, cols, MASKS[mi], R))
        assert counts["hole"] + counts["source"] + counts["bystander"] == rows * cols
        filled += counts["filled"]; bystanders += counts["bystander"]
        nan_kept += int((np.isnan(want[1]) & np.isnan(depth)).sum())
    if rows * cols > 1000:
        assert arity == {1, 2, 3, 4}                                         # the random masks met every count of valid children
        assert filled > 1000 and bystanders > 100 and nan_kept > 10


def test_wild_depths_are_clamped_before_they_are_compared_or_averaged():
    rows, cols = 12, 10
    orig = inputs(37, 53)[0][:rows, :cols]
    depth = np.full((rows, cols), 300.0, F); depth[:, :3] = -50.0; depth[0, 5] = np.nan; depth[1, 5] = np.inf; depth[2, 5] = -np.inf
    mask = np.zeros((rows, cols), np.uint8); mask[4:8, 4:8] = 1
    for limit in (0.0, 100.0, 255.0):
        R = removal(0, 0, limit)
        got = remove(orig, depth, mask, R)
        assert_same(remove_literal(orig, depth, mask, R), got, limit)
        assert (got[1][4:8, 4:8] <= 255).all() and (got[1][4:8, 4:8] >= 0).all()     # averages of clamped depths
        if limit >= 100:
            assert (got[1][4:8, 4:8] == 255).all()                           # only the far pixels (300 -> 255) were sources
    keep = np.ones((rows, cols), bool); keep[4:8, 4:8] = False
    assert same_bits(got[1][keep], depth[keep])                              # NaN, inf and the rest: bits copied


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_identities(rows, cols):
    orig, depth = inputs(rows, cols)
    rng = np.random.default_rng(5)
    for R in (removal(0, 8, 0.0), removal(CODE, 3, 100.0)):
        # no selected pixel: a mask of zeros, and a code no pixel carries
        assert_same(remove(orig, depth, np.zeros((rows, cols), np.uint8), R), (orig, depth), "mask all zero")
        assert_same(remove(orig, depth, np.full((rows, cols), OTHER, np.uint8), removal(CODE, R["grow"], R["sourceMinDepth"])), (orig, depth), "no selection")
        # no source anywhere: everything a hole
        assert_same(remove(orig, depth, np.full((rows, cols), CODE, np.uint8), R), (orig, depth), "no source")
    # every source one colour: the hole takes exactly that colour
    flat = np.empty_like(orig); flat[...] = (13, 200, 77)
    mask = (rng.random((rows, cols)) < 0.6).astype(np.uint8)
    art, _ = remove(flat, depth, mask, removal(0, 1, 0.0))
    assert np.array_equal(art, flat)
    # all but pixel (0, 0) a hole: the whole image takes that pixel's colour (and depth 40 is 40 after every 16 d / 16)
    d40 = np.full((rows, cols), 40.0, F)
    art, z = remove(orig, d40, mask_pattern("allbut", rows, cols), removal(CODE, 0, 0.0))
    assert (art == orig[0, 0]).all() and (z == 40).all()


def test_a_grown_ring_never_covers_a_nearer_pixel():
    rows, cols = 37, 53
    orig, depth = inputs(rows, cols)
    mask = mask_pattern("borders", rows, cols)
    sel = selected(mask, CODE)
    near = ~(np.nan_to_num(depth, nan=0.0) >= 100)                           # d' < 100 (a NaN is 0)
    for grow in GROWS:
        hole, source = classes(depth, mask, removal(CODE, grow, 100.0))
        assert not (hole & ~sel & near).any() and not (source & near).any()
        art, z = remove(orig, depth, mask, removal(CODE, grow, 100.0))
        keep = ~sel & near
        assert np.array_equal(art[keep], orig[keep]) and same_bits(z[keep], depth[keep])
    assert (classes(depth, mask, removal(CODE, 8, 100.0))[0] & ~sel).sum() > 50          # the ring exists where it may


def test_lift_restated_per_texel():
    rows, cols = 9, 11
    orig = inputs(37, 53)[0][:rows, :cols]
    mask = mask_pattern("random", rows, cols, seed=2)
    for select in (0, CODE):
        for (x, y, sr, sc) in ((2, 3, 4, 5), (-3, -2, 6, 7), (8, 6, 5, 6), (-2, -2, 14, 16), (20, 3, 4, 4), (3, -9, 5, 5)):
            got = lift(orig, mask, select, x, y, sr, sc)
            for v in range(sr):
                for u in range(sc):
                    py, px = y + v, x + u
                    inside = 0 <= py < rows and 0 <= px < cols
                    on = inside and (mask[py, px] != 0 if select == 0 else mask[py, px] == select)
                    assert tuple(got[v, u]) == ((*orig[py, px], 255) if on else (0, 0, 0, 0))


@pytest.mark.parametrize("limit", [0.0, 100.0, 255.0])
def test_lift_remove_composite_gives_the_original_back(limit):
    rows, cols = 37, 53
    orig, depth = inputs(rows, cols)
    mask = np.zeros((rows, cols), np.uint8)
    mask[5:30, 10:40] = mask_pattern("disc", 25, 30)
    mask[33, 2] = OTHER
    x, y, sr, sc = 8, 3, 30, 36                                              # a box that covers the selection
    sprite = lift(orig, mask, CODE, x, y, sr, sc)
    assert (sprite[..., 3] == 255).sum() == (mask == CODE).sum() > 100
    art, z = remove(orig, depth, mask, removal(CODE, 0, limit))
    assert not np.array_equal(art, orig)
    L = layer(sr, sc, x, y, 256, NEAREST, 255, depth0=0.0, depth1=0.0, feather=0.0)
    back, zb = composite(art, z, sprite, L)
    assert np.array_equal(back, orig)
    assert (zb[mask == CODE] == 0).all() and same_bits(zb[mask != CODE], z[mask != CODE])


def disc_hole(rows, cols, rad):
    """The issue's six discs: centres from default_rng(1), rows first."""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:rows, 0:cols]
    hole = np.zeros((rows, cols), bool)
    for _ in range(6):
        cy = int(rng.integers(rad, rows - rad)); cx = int(rng.integers(rad, cols - rad))
        hole |= (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
    return hole


@pytest.mark.parametrize("name", ["Dog", "Hills", "Flower"])
def test_push_pull_beats_the_nearest_pixel_of_the_row(name):
    bgr = load_pair(name)[0]
    rows, cols = bgr.shape[:2]
    depth = np.full((rows, cols), 128.0, F)
    for rad in (8, 24, 64):
        hole = disc_hole(rows, cols, rad)
        art, _ = remove(bgr, depth, hole.astype(np.uint8), removal())
        err = lambda a: float(np.abs(a[hole].astype(np.int64) - bgr[hole].astype(np.int64)).mean())       # noqa: E731
        pp, row = err(art), err(nearest_in_row(bgr, hole))
        print(f"{name} radius {rad}: push-pull {pp:.1f}, nearest in row {row:.1f}")
        assert pp < row


def two_box_scene():
    rows, cols = 48, 64
    yy, xx = np.mgrid[0:rows, 0:cols]
    back = np.stack([40 + 2 * xx, 200 - 2 * yy, np.full_like(xx, 90)], -1).astype(np.uint8)
    orig = back.copy(); depth = np.full((rows, cols), 200.0, F)
    orig[12:36, 16:36] = 255; depth[12:36, 16:36] = 40
    orig[8:40, 36:48] = (0, 0, 255); depth[8:40, 36:48] = 60
    mask = np.zeros((rows, cols), np.uint8); mask[12:36, 16:36] = 1
    return orig, depth, mask, back


def test_the_source_limit_keeps_a_nearer_neighbour_out_of_the_fill():
    orig, depth, mask, back = two_box_scene()
    hole = mask != 0
    err = {}
    for limit in (0.0, 100.0):
        art, z = remove(orig, depth, mask, removal(0, 0, limit))
        err[limit] = float(np.abs(art[hole].astype(np.int64) - back[hole].astype(np.int64)).mean())
        print(f"sourceMinDepth {limit}: error {err[limit]:.2f}, filled depth {z[hole].min():.1f} .. {z[hole].max():.1f}")
        if limit == 100.0:
            assert (z[hole] == 200).all()
            assert np.array_equal(art[~hole], orig[~hole])                   # the red box is a bystander: kept
    assert err[100.0] < err[0.0]


def test_the_c_abi_lists_both_entry_points():
    assert "rtdd_remove_object" in rt.C_ABI_SYMBOLS and "rtdd_lift_layer" in rt.C_ABI_SYMBOLS


def test_the_plan_mirrors_the_constants():
    T, G, A = rt.REMOVE_TILE, rt.REMOVE_GROUP, rt.REMOVE_APEX
    assert T == 1 << (G + 3) and A * 8 * 3 // 2 + 64 * 8 <= 160 * 1024       # the apex's chain, 8 B a sample, fits one workgroup's LDS
    assert rt.remove_plan(1, 1) == [(0, 1, 1)] and rt.remove_plan(3, 2) == [(2, 1, 1)]
    side = int(A ** 0.5) << G                                                # the largest square whose third level the apex takes
    assert len(rt.remove_plan(side, side)) == 1 and len(rt.remove_plan(side + 1, side + 1)) == 2
    assert len(rt.remove_plan(730, 730)) == 2 and len(rt.remove_plan(1080, 1920)) == 2 and len(rt.remove_plan(4320, 7680)) == 2
