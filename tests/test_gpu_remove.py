"""rtdd_remove_object and rtdd_lift_layer (include/rtdd.h) on the GPU (-m gpu): byte for byte, and on the depth bit for bit, against the
numpy restatement of tests/remove_ref.py, which knows nothing of the kernels (no tiles, no groups, no apex).  The shapes come from the
grouping's constants (rt.REMOVE_TILE, rt.REMOVE_GROUP, rt.REMOVE_APEX) and each asserts the path it takes: one tile and more, ragged
tiles, odd sizes at every level, the largest square one pull group serves and the smallest that needs two.  Every hole pattern, grow,
select and source limit of the issue, pairwise on every shape; depth maps with values outside [0, 255] and NaN; copies; depthOut NULL; sub-image views
of every pointer; behind an unsynchronised estimate; the heal log; the refusals; the lift; the lift / remove / composite identity; the
chain into an effect that reads the removal's depth map.  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd import REMOVE_APEX, REMOVE_GROUP, REMOVE_TILE, Layer, Removal        # (absent without the feature)
from composite_ref import NEAREST, composite, layer
from dataset_util import load_pair
from effect_gpu import ctx  # noqa: F401
from effect_gpu import FILL, assert_same_image, clean_and_healed, estimate, random_inputs, raw_images
from gpu_util import down, up
from relight_ref import light
from remove_ref import CODE, OTHER, lift, mask_pattern, remove, removal, same_bits
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from shadow_ref import relight_shadowed, shadow

pytestmark = pytest.mark.gpu

ZFILL = -7.0                                     # what a depthOut image holds before the call writes it
T, G, A = REMOVE_TILE, REMOVE_GROUP, REMOVE_APEX
ONE_GROUP = int(A ** 0.5) << G                   # the largest square whose level G the apex takes (720 with 64 / 3 / 8192)
# one tile and four; the largest square one pull group serves and the smallest that needs two (721 with 64 / 3 / 8192: ceil(721 / 8) = 91
# and 91 * 91 > 8192), and the issue's 730, which needs two as well
SHAPES = [(1, 1), (1, 7), (9, 1), (37, 53), (T, T), (T + 1, T + 1), (257, 513), (ONE_GROUP, ONE_GROUP), (ONE_GROUP + 1, ONE_GROUP + 1), (730, 730)]
MASKS = ["random", "checker", "disc", "borders", "allbut", "tileedge"]
GROWS = [0, 1, 3, 8]
SELECTS = [0, CODE]
LIMITS = [0.0, 100.0]


def up_level(n, times):
    for _ in range(times):
        n = (n + 1) // 2
    return n


def groups_expected(rows, cols):
    """How many pull groups the constants give a rows x cols image: levels go G at a time until one has at most A samples."""
    n = 1
    while up_level(rows, G * n) * up_level(cols, G * n) > A:
        n += 1
    return n


def make_mask(name, rows, cols, seed=0):
    """remove_ref's patterns, and "tileedge": single selected pixels 0, 3 and 7 away from the first tile border, on both sides of it, in
    x and in y (so a ring of up to 8 crosses the border from either side)."""
    if name != "tileedge":
        return mask_pattern(name, rows, cols, seed)
    m = np.zeros((rows, cols), np.uint8)
    for i, k in enumerate((0, 3, 7)):
        for p in (T - 1 - k, T + k):
            if p < cols:
                m[min(5 + 20 * i, rows - 1), p] = CODE
            if p < rows:
                m[p, min(9 + 20 * i, cols - 1)] = CODE
    m[rows // 2, cols // 2] = CODE
    return m


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols):
    orig, depth = random_inputs(rows, cols, rows * 1000 + cols)              # depths in [-20, 275], 3 % NaN
    return orig, depth


def _remove(c, o, d, m, rows, cols, R, with_depth=True):
    """rtdd_remove_object into fresh outputs.  Returns (artistic, depthOut or None) on the host."""
    art = up(np.full((rows, cols, 3), FILL, np.uint8))
    z = up(np.full((rows, cols), ZFILL, np.float32)) if with_depth else None
    c.remove_object(o, d, m, art, z, rows, cols, Removal(**R))
    c.synchronize()
    return down(art), (down(z) if with_depth else None)


def assert_same(got, want, what):
    assert_same_image(got[0], want[0], what)
    assert same_bits(got[1], want[1]), f"{what}: {int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())} depths differ"


# The full pairwise set runs on every shape.  A shape above 100000 pixels, whose restatement takes longest, is split into one test id per
# mask: together the ids of a shape are the whole set, and each holds every grow, select and source limit.
CASES = [(r, c, None) for r, c in SHAPES if r * c <= 100000] + [(r, c, m) for r, c in SHAPES if r * c > 100000 for m in MASKS]


@pytest.mark.parametrize("rows,cols,only", CASES, ids=lambda v: str(v))
def test_parameters_bit_exact(ctx, rows, cols, only):
    """Every pair of levels of mask, grow, select and source limit occurs (roi_util.covering) on every shape."""
    plan = rt.remove_plan(rows, cols)
    assert len(plan) == groups_expected(rows, cols) == (2 if rows > ONE_GROUP else 1)
    assert plan[-1][1] * plan[-1][2] <= A and (len(plan) == 1 or plan[-2][1] * plan[-2][2] > A)
    assert plan[0][0] == min(G, (max(rows, cols) - 1).bit_length()) and plan[0][1:] == (up_level(rows, plan[0][0]), up_level(cols, plan[0][0]))
    orig, depth = _inputs(rows, cols)
    o, d = up(orig), up(depth)
    combos = [cb for cb in covering(len(MASKS), len(GROWS), len(SELECTS), len(LIMITS)) if only is None or MASKS[cb[0]] == only]
    assert {cb[1] for cb in combos} == set(range(len(GROWS))) and {cb[2:] for cb in combos} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    filled = bystanders = nan_kept = 0
    for mi, gi, si, li in combos:
        mask = make_mask(MASKS[mi], rows, cols, seed=mi + 1)
        R = removal(SELECTS[si], GROWS[gi], LIMITS[li])
        counts = {}
        want = remove(orig, depth, mask, R, counts)
        got = _remove(ctx, o, d, up(mask), rows, cols, R)
        assert_same(got, want, (rows, cols, MASKS[mi], R))
        filled += counts["filled"]; bystanders += counts["bystander"]
        nan_kept += int((np.isnan(want[1]) & np.isnan(depth)).sum())
    if rows * cols > 1000:
        assert filled > 1000 and nan_kept > 10                               # holes were filled, NaN bits were copied
        assert bystanders > 100 or only == "allbut"                          # bystanders existed (all but one pixel a hole leaves room for one)


@pytest.mark.parametrize("rows,cols", [(37, 53), (T + 1, T + 1), (257, 513)], ids=lambda v: str(v))
def test_all_hole_and_no_hole_copy(ctx, rows, cols):
    orig, depth = _inputs(rows, cols)
    o, d = up(orig), up(depth)
    for name, R in (("all", removal(CODE, 8, 0.0)), ("none", removal(0, 8, 0.0)), ("random", removal(200, 3, 0.0))):     # (no pixel carries 200)
        got = _remove(ctx, o, d, up(make_mask(name, rows, cols)), rows, cols, R)
        assert_same(got, (orig, depth), name)
    flat = np.empty_like(orig); flat[...] = (13, 200, 77)                    # one colour: the fill is that colour exactly
    got = _remove(ctx, up(flat), d, up(make_mask("random", rows, cols)), rows, cols, removal(0, 1, 0.0))
    assert_same_image(got[0], flat, "one colour")


def test_depth_out_null_writes_nothing_but_artistic(ctx):
    rows, cols = 130, 200
    orig, depth = _inputs(rows, cols)
    mask = make_mask("disc", rows, cols)
    o, d, m = up(orig), up(depth), up(mask)
    R = removal(CODE, 3, 100.0)
    want = remove(orig, depth, mask, R)
    art, z = _remove(ctx, o, d, m, rows, cols, R, with_depth=False)
    assert z is None
    assert_same_image(art, want[0], "depthOut NULL")
    assert not np.array_equal(art, orig)
    assert same_bits(down(d), depth) and np.array_equal(down(o), orig) and np.array_equal(down(m), mask)


# (lead, pitch residue) indices of the original, the depth map, the mask, the artistic image and depthOut
@pytest.mark.parametrize("layout", [(0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 3, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, 0, 3), (3, 3, 5, 4, 6)],
                         ids=["aligned", "original", "depth", "mask", "artistic", "depthOut", "all"])
@pytest.mark.parametrize("rows,cols", [(37, 53), (130, 200)], ids=lambda v: str(v))
def test_sub_image_views(ctx, rows, cols, layout):
    orig, depth = _inputs(rows, cols)
    mask = make_mask("disc", rows, cols)
    (lo, ro), (ld, rd), (lm, rm), (la, ra), (lz, rz) = (LAYOUTS_U8[layout[0]], LAYOUTS_F32[layout[1]], LAYOUTS_U8[layout[2]], LAYOUTS_U8[layout[3]],
                                                        LAYOUTS_F32[layout[4]])
    o = Roi(orig, lo, pitch_for(cols * 3, lo, ro), FILL_INPUT, what="original")
    d = Roi(depth, ld, pitch_for(cols * 4, ld, rd), FILL_INPUT, what="depth")
    m = Roi(mask, lm, pitch_for(cols, lm, rm), FILL_INPUT, what="mask")
    out = Roi(np.zeros_like(orig), la, pitch_for(cols * 3, la, ra), FILL_OUTPUT, seed=5, what="artistic")
    zout = Roi(np.zeros_like(depth), lz, pitch_for(cols * 4, lz, rz), FILL_OUTPUT, seed=6, what="depthOut")
    # select CODE with the widest ring, and select 0, under which the 0xFF bytes around the mask's view would count as selected: a read
    # of the lead or of the row padding changes the hole
    for R in (removal(CODE, 8, 0.0), removal(0, 3, 0.0), removal(0, 0, 100.0)):
        ctx.remove_object(o.img, d.img, m.img, out.img, zout.img, rows, cols, Removal(**R))
        ctx.synchronize()
        assert_same((out.result(), zout.result()), remove(orig, depth, mask, R), (rows, cols, layout, R))
        o.assert_unchanged(); d.assert_unchanged(); m.assert_unchanged()
    # the sprite of a lift is a view too
    sr, sc = 40, 61
    sp = Roi(np.zeros((sr, sc * 4), np.uint8), la, pitch_for(sc * 4, la, ra), FILL_OUTPUT, seed=7, what="sprite")
    for select in (CODE, 0):
        ctx.lift_layer(o.img, m.img, rows, cols, select, -5, 10, sp.img, sr, sc)
        ctx.synchronize()
        assert np.array_equal(sp.result().reshape(sr, sc, 4), lift(orig, mask, select, -5, 10, sr, sc))
    o.assert_unchanged(); m.assert_unchanged()


def test_queued_behind_an_unsynchronised_estimate():
    bgr, ann, _ = load_pair("Dog")
    rows, cols = bgr.shape[:2]
    mask = make_mask("disc", rows, cols)
    R = removal(CODE, 3, 60.0)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        o, m = up(bgr), up(mask)
        art, z = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), np.float32))
        d = estimate(c, bgr, ann)
        c.remove_object(o, d, m, art, z, rows, cols, Removal(**R))          # no synchronisation since the estimate was queued
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        want = remove(bgr, depth, mask, R)
        assert_same((down(art), down(z)), want, "behind an estimate")
    assert not np.array_equal(want[0], bgr) and not same_bits(want[1], depth)


def test_remove_and_lift_are_replayed_after_a_healed_solve():
    rows, cols = 130, 200
    orig = _inputs(rows, cols)[0]
    mask = make_mask("disc", rows, cols)
    R = removal(CODE, 1, 0.5)
    x, y, sr, sc = 20, 2, 120, 170
    L = layer(sr, sc, x + 15, y, 256, NEAREST, 255, depth0=0.0, depth1=0.0)  # the object, moved 15 to the right
    kept = []

    def queue(c, o, d, arts):
        m, z = up(mask), up(np.full((rows, cols), ZFILL, np.float32))
        s = up(np.full((sr, sc, 4), FILL, np.uint8))
        kept.append((m, z, s))
        c.remove_object(o, d, m, arts[0], z, rows, cols, Removal(**R))
        c.lift_layer(o, m, rows, cols, CODE, x, y, s, sr, sc)
        c.composite_layer(arts[0], z, s, arts[1], None, rows, cols, Layer(**L))

    solved, healed = clean_and_healed(queue, 2, orig)
    want = remove(orig, solved, mask, R)
    assert_same((healed[0], down(kept[1][1])), want, "healed")
    assert same_bits(down(kept[0][1]), want[1])
    sprite = lift(orig, mask, CODE, x, y, sr, sc)
    assert np.array_equal(down(kept[1][2]), sprite)
    assert_same_image(healed[1], composite(want[0], want[1], sprite, L)[0], "healed: the object moved")
    assert not np.array_equal(healed[0], orig)


def _raw_remove(c, o, d, m, art, z, rows, cols, R, override):
    po, op, pd, dp, pa, ap = raw_images(o, d, art)
    a = dict(ctx=c._h, original=po, originalPitch=op, depth=pd, depthPitch=dp, mask=C.c_void_p(m.data_ptr()), maskPitch=C.c_size_t(m.stride(0)),
             artistic=pa, artisticPitch=ap, depthOut=C.c_void_p(z.data_ptr()), depthOutPitch=C.c_size_t(z.stride(0) * 4), rows=rows, cols=cols,
             removal=C.byref(R) if R is not None else None)
    a.update(override)
    return rt.lib().rtdd_remove_object(*a.values())


def _raw_lift(c, o, m, s, rows, cols, override):
    a = dict(ctx=c._h, original=C.c_void_p(o.data_ptr()), originalPitch=C.c_size_t(o.stride(0)), mask=C.c_void_p(m.data_ptr()), maskPitch=C.c_size_t(m.stride(0)),
             rows=rows, cols=cols, select=0, x=2, y=3, sprite=C.c_void_p(s.data_ptr()), spritePitch=C.c_size_t(s.stride(0)), spriteRows=9,
             spriteCols=7)
    a.update(override)
    return rt.lib().rtdd_lift_layer(*a.values())


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 37, 53
    orig, depth = _inputs(rows, cols)
    mask = make_mask("random", rows, cols)
    good = removal(CODE, 3, 100.0)
    with rt.Context(0) as c:
        o, d, m = up(orig), up(depth), up(mask)
        art, z = up(np.full_like(orig, FILL)), up(np.full((rows, cols), ZFILL, np.float32))
        s = up(np.full((9, 7, 4), FILL, np.uint8))
        po, op, pd, dp, pa, ap = raw_images(o, d, art)
        pz, zp = z.data_ptr(), z.stride(0) * 4
        images = {"null context": dict(ctx=None), "null original": dict(original=None), "null depth": dict(depth=None), "null artistic": dict(artistic=None),
                  "original pitch short of a row": dict(originalPitch=C.c_size_t(cols * 3 - 1)), "depth pitch short of a row": dict(depthPitch=C.c_size_t(cols * 4 - 4)),
                  "artistic pitch short of a row": dict(artisticPitch=C.c_size_t(cols * 3 - 1)), "depthOut pitch short of a row": dict(depthOutPitch=C.c_size_t(cols * 4 - 4)),
                  "depth pitch no multiple of 4": dict(depthPitch=C.c_size_t(dp.value + 2)), "depth pointer off by 2 bytes": dict(depth=C.c_void_p(pd.value + 2)),
                  "depthOut pitch no multiple of 4": dict(depthOutPitch=C.c_size_t(zp + 2)), "depthOut pointer off by 2 bytes": dict(depthOut=C.c_void_p(pz + 2)),
                  "negative rows": dict(rows=-1), "negative cols": dict(cols=-1), "rows^2 + cols^2 >= 2^31": dict(rows=40000, cols=40000),
                  "original == artistic": dict(artistic=po, artisticPitch=op), "depth == depthOut": dict(depthOut=pd, depthOutPitch=dp),
                  "null mask": dict(mask=None), "mask pitch short of a row": dict(maskPitch=C.c_size_t(cols - 1)), "null removal": dict(removal=None)}
        for what, override in images.items():
            assert _raw_remove(c, o, d, m, art, z, rows, cols, Removal(**good), override) == 1, what
        assert _raw_remove(c, o, d, m, art, z, rows, cols, Removal(**good), dict(rows=0)) == 0                 # (the call itself is sound: an empty image)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(select=-1), dict(select=256), dict(grow=-1), dict(grow=9), dict(sourceMinDepth=-0.5), dict(sourceMinDepth=255.5),
                   dict(sourceMinDepth=nan), dict(sourceMinDepth=inf), dict(sourceMinDepth=-inf)):
            with pytest.raises(rt.RtddError) as e:
                c.remove_object(o, d, m, art, z, rows, cols, Removal(**dict(good, **kw)))
            assert e.value.status == 1, kw
        lifts = {"null context": dict(ctx=None), "null original": dict(original=None), "null mask": dict(mask=None), "null sprite": dict(sprite=None),
                 "original pitch short of a row": dict(originalPitch=C.c_size_t(cols * 3 - 1)), "mask pitch short of a row": dict(maskPitch=C.c_size_t(cols - 1)),
                 "sprite pitch short of a row": dict(spritePitch=C.c_size_t(7 * 4 - 1)), "negative rows": dict(rows=-1), "negative cols": dict(cols=-1),
                 "rows^2 + cols^2 >= 2^31": dict(rows=40000, cols=40000), "select -1": dict(select=-1), "select 256": dict(select=256),
                 "x low": dict(x=-16385), "x high": dict(x=16384), "y low": dict(y=-16385), "y high": dict(y=16384),
                 "no sprite rows": dict(spriteRows=0), "no sprite cols": dict(spriteCols=0), "too many sprite rows": dict(spriteRows=16385),
                 "too many sprite cols": dict(spriteCols=16385, spritePitch=C.c_size_t(1 << 20)), "in place": dict(sprite=C.c_void_p(o.data_ptr()))}
        for what, override in lifts.items():
            assert _raw_lift(c, o, m, s.flatten(1), rows, cols, override) == 1, what
        c.synchronize()
        assert (down(art) == FILL).all() and (down(z) == ZFILL).all() and (down(s) == FILL).all()             # nothing was launched
        # the limits themselves are accepted
        for kw in (dict(select=255, grow=8, sourceMinDepth=255.0), dict(select=0, grow=0, sourceMinDepth=0.0)):
            R = dict(good, **kw)
            c.remove_object(o, d, m, art, z, rows, cols, Removal(**R))
            c.synchronize()
            assert_same((down(art), down(z)), remove(orig, depth, mask, R), kw)
        c.remove_object(o, d, m, art, z, 0, cols, Removal(**good))           # an empty image: nothing to do
        for x, y in ((-16384, 16383), (16383, -16384)):
            c.lift_layer(o, m, rows, cols, 255, x, y, s, 9, 7)
            c.synchronize()
            assert (down(s) == 0).all()


@pytest.mark.parametrize("rows,cols", [(37, 53), (130, 300)], ids=lambda v: str(v))
def test_lift_layer_inside_across_and_outside(ctx, rows, cols):
    orig = _inputs(rows, cols)[0]
    mask = make_mask("random", rows, cols, seed=4)
    o, m = up(orig), up(mask)
    sr, sc = 21, 30
    boxes = [(5, 4), (-sc // 2, 6), (cols - sc // 2, 6), (7, -sr // 2), (7, rows - sr // 2), (-sc // 2, -sr // 2), (cols - 3, rows - 2),
             (-40 * sc, 3), (cols, 3), (3, -sr), (3, rows + 1)]              # inside; across each border and two corners; wholly outside
    lifted = 0
    for select in (0, CODE, OTHER):
        for x, y in boxes:
            s = up(np.full((sr, sc, 4), FILL, np.uint8))
            ctx.lift_layer(o, m, rows, cols, select, x, y, s, sr, sc)
            ctx.synchronize()
            want = lift(orig, mask, select, x, y, sr, sc)
            assert np.array_equal(down(s), want), (select, x, y)
            lifted += int(want[..., 3].any())
    big_r, big_c = rows + 9, cols + 300                                      # wider than a wave's span, the image inside it
    s = up(np.full((big_r, big_c, 4), FILL, np.uint8))
    ctx.lift_layer(o, m, rows, cols, 0, -150, -4, s, big_r, big_c)
    ctx.synchronize()
    assert np.array_equal(down(s), lift(orig, mask, 0, -150, -4, big_r, big_c))
    assert lifted >= 3 * 5                                                   # (a corner box of a few pixels may hold no selected one)


@pytest.mark.parametrize("limit", [0.0, 100.0])
def test_lift_remove_composite_gives_the_original_back(ctx, limit):
    rows, cols = 130, 200
    orig, depth = _inputs(rows, cols)
    mask = make_mask("disc", rows, cols); mask[3, 190] = OTHER
    ys, xs = np.nonzero(mask == CODE)
    x, y, sr, sc = int(xs.min()) - 2, int(ys.min()), int(ys.max() - ys.min()) + 1, int(xs.max() - xs.min()) + 5
    o, d, m = up(orig), up(depth), up(mask)
    art, z = up(np.zeros_like(orig)), up(np.zeros_like(depth))
    s, back, zb = up(np.zeros((sr, sc, 4), np.uint8)), up(np.zeros_like(orig)), up(np.zeros_like(depth))
    ctx.lift_layer(o, m, rows, cols, CODE, x, y, s, sr, sc)
    ctx.remove_object(o, d, m, art, z, rows, cols, Removal(CODE, 0, limit))
    ctx.composite_layer(art, z, s, back, zb, rows, cols, Layer(**layer(sr, sc, x, y, 256, NEAREST, 255)))
    ctx.synchronize()
    assert not np.array_equal(down(art), orig)
    assert_same_image(down(back), orig, "lift, remove, composite")
    assert (down(zb)[mask == CODE] == 0).all()


def test_chain_into_the_shadowed_relight(ctx):
    """remove, then rtdd_simulate_relight_shadowed on (artistic, depthOut): the restatements chained.  The box no longer casts a shadow."""
    rows, cols = 60, 80
    rng = np.random.default_rng(9)
    orig = rng.integers(40, 256, (rows, cols, 3), dtype=np.uint8)
    depth = np.full((rows, cols), 200, np.float32); depth[10:50, 28:44] = 40; depth += rng.uniform(-3, 3, (rows, cols)).astype(np.float32)
    mask = np.zeros((rows, cols), np.uint8); mask[10:50, 28:44] = 1
    R = removal(0, 2, 100.0)
    o, d, m = up(orig), up(depth), up(mask)
    art, z, lit = up(np.zeros_like(orig)), up(np.zeros_like(depth)), up(np.zeros_like(orig))
    Lt, S = light(x=-1.0, y=0.2, z=1.0, relief=0.1, ambient=0.2), shadow(maxSteps=64, bias=0.25)
    ctx.remove_object(o, d, m, art, z, rows, cols, Removal(**R))
    ctx.simulate_relight_shadowed(art, z, lit, rows, cols, rt.Light(**Lt), rt.Shadow(**S))
    ctx.synchronize()
    want = remove(orig, depth, mask, R)
    assert_same((down(art), down(z)), want, "remove")
    assert (want[1][10:50, 28:44] > 190).all()                               # the box's depth is the wall's now
    assert_same_image(down(lit), relight_shadowed(want[0], want[1], Lt, S), "relight_shadowed on the removal")
    assert not np.array_equal(down(lit), relight_shadowed(want[0], depth, Lt, S))       # the depth map matters


# ---- the harness: --remove-region and --move-region on the region --region-fill paints -------------------------------------------------
REGION = [(250, 150), (400, 160), (390, 330), (260, 320)]


@pytest.fixture(scope="module")
def harness_scene(tmp_path_factory):
    """The harness's own estimate with region 3 painted, through the library: (directory, bgr, depth, the level-0 region codes)."""
    from effect_gpu import harness_pair
    import polygon_ref as pr
    tmp = tmp_path_factory.mktemp("remove_harness")
    bgr, ann = harness_pair(tmp, "pnm")
    rows, cols = bgr.shape[:2]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.pyramid_set_regions(rt.REGION_CUT)
        c.fill_polygon(REGION, pr.constant(3), c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], rows, cols)
        c.estimate_depth(1000)
        c.synchronize()
        depth, codes = c.pyramid_download(rt.IMG_DEPTH, 0), c.pyramid_download(rt.IMG_REGION_CODE, 0)
    assert (codes == 3).sum() > 10000 and set(np.unique(codes)) == {0, 3}
    return tmp, bgr, depth, codes


REGION_ARGS = ["--regions", "cut", "--region-fill", ";".join(f"{x},{y}" for x, y in REGION) + ":3"]


def test_harness_remove_region(harness_scene):
    from effect_gpu import run_harness
    tmp, bgr, depth, codes = harness_scene
    got = run_harness(tmp, "pnm", REGION_ARGS + ["--remove-region", "3", "--remove-grow", "4", "--remove-behind", "20"])[1]
    want = remove(bgr, depth, codes, removal(3, 4, 20.0))
    assert not np.array_equal(want[0], bgr)
    assert_same_image(got, want[0], "harness: --remove-region")
    # --effect then runs on the removal and its depth map
    from refocus_ref import refocus_by_summed_area_table
    got = run_harness(tmp, "pnm", REGION_ARGS + ["--remove-region", "3", "--effect", "refocus", "--focus", "128"])[1]
    want = remove(bgr, depth, codes, removal(3, 0, 0.0))
    assert_same_image(got, refocus_by_summed_area_table(want[0], want[1], 128.0), "harness: remove, then refocus")


def test_harness_move_region(harness_scene):
    from effect_gpu import run_harness
    tmp, bgr, depth, codes = harness_scene
    rows, cols = codes.shape
    sprite = lift(bgr, codes, 3, 0, 0, rows, cols)
    art, z = remove(bgr, depth, codes, removal(3, 0, 0.0))
    for tail, zl in ((":40", 40.0), ("", float(np.clip(np.nan_to_num(depth[codes == 3]), 0, 255).min()))):
        got = run_harness(tmp, "pnm", REGION_ARGS + ["--move-region", "3:-60,25" + tail])[1]
        want = composite(art, z, sprite, layer(rows, cols, -60, 25, 256, NEAREST, 255, depth0=zl, depth1=zl))[0]
        assert not np.array_equal(want, art)
        assert_same_image(got, want, f"harness: --move-region {tail}")


def test_harness_refuses_a_removal_it_cannot_do(tmp_path):
    import subprocess
    from effect_gpu import harness_bin
    for args, text in ((["--live", "3", "--regions", "cut", "--remove-region", "3"], "not supported with --live"),
                       (["--remove-region", "3"], "need --regions"), (["--remove-grow", "2"], "need --remove-region"),
                       (["--regions", "cut", "--remove-region", "3", "--move-region", "3:1,1"], "one at a time"),
                       (["--regions", "cut", "--move-region", "3"], "--move-region wants"), (["--regions", "cut", "--remove-region", "0"], "1..255")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (args, r.stdout)
