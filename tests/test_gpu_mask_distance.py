"""rtdd_mask_distance, rtdd_refine_mask and rtdd_lift_layer_matte (include/rtdd.h) on the GPU (-m gpu): word for word and byte for byte
against tests/mask_distance_ref.py, which knows nothing of the kernels.  The shapes come from the exported geometry (rt.EDT_TILE_W,
rt.EDT_TILE_H, rt.EDT_BAND, rt.EDT_LDS_REACH); the masks put single pixels around
the first tile and band borders at the distances where a reach ends; the reaches straddle a word of the column pass and the largest halo
staged in LDS, and 1024 is on these shapes the unbounded transform (tests/mask_distance_cases.py holds the three lists, and
tests/test_mask_distance_cpu.py checks the reference used here against a second route on every one of them).  rt.mask_distance_plan
mirrors the launcher's choice of path as rt.remove_plan mirrors its plan: the tests assert that the plan names the path each reach is meant
to take and that both paths were asked for, not which instantiation the library launched.  Every output is a sub-image view whose surroundings are checked
(roi_util).  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd import (DISTANCE_FAR, EDT_BAND, EDT_LDS_REACH, EDT_TILE_H, EDT_TILE_W, REFINE_FEATHER, REFINE_GROW,        # (absent
                                        REFINE_OUTLINE, REFINE_SHRINK, MaskRefine, mask_distance_plan)                                     # without the feature)
import mask_distance_cases as cases
import mask_distance_ref as mr
from mask_distance_cases import MASKS, REACHES, SELECTS, SHAPES, make_mask        # (shared with tests/test_mask_distance_cpu.py, which checks the reference on them)
from composite_ref import NEAREST, composite, layer
from effect_gpu import ctx  # noqa: F401
from effect_gpu import FILL, assert_same_image, clean_and_healed, estimate, random_inputs
from dataset_util import load_pair
from gpu_util import down, up
from remove_ref import CODE, lift, same_bits
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for

pytestmark = pytest.mark.gpu

W, H, B, L = EDT_TILE_W, EDT_TILE_H, EDT_BAND, EDT_LDS_REACH
assert (W, H, B, L) == (cases.W, cases.H, cases.B, cases.L)
assert DISTANCE_FAR == mr.FAR and (REFINE_GROW, REFINE_SHRINK, REFINE_OUTLINE, REFINE_FEATHER) == (mr.GROW, mr.SHRINK, mr.OUTLINE, mr.FEATHER)
LOHI = [-1023.5, -7.25, -1.0, -0.5, 0.0, 0.5, 1.0, 7.25, 1023.5]


@functools.lru_cache(maxsize=None)
def _case(name, rows, cols, select, reach_key):
    """(mask, selected, E): computed once per case and shared; never modified (the reference's arrays are read-only; the mask is what
    torch uploads, which wants a writable array)."""
    m = make_mask(name, rows, cols, reach_key)
    sel = mr.selected(m, select)
    E = mr.e_scipy(sel)
    for a in (sel, E):
        a.setflags(write=False)
    return m, sel, E


def case(name, rows, cols, select, reach):
    assert name != "edges" or reach in cases.EDGE_REACHES                   # (the reference is checked on exactly these)
    return _case(name, rows, cols, select, reach if name == "edges" else 0)


def out_roi(rows, cols, dtype, layout=(0, 0), seed=1, what="out"):
    width = cols * np.dtype(dtype).itemsize
    return Roi(np.zeros((rows, cols), dtype), layout[0], pitch_for(width, *layout), FILL_OUTPUT, seed=seed, what=what)


def gpu_distance(c, mask_img, rows, cols, select, reach, layout=(0, 0)):
    d = out_roi(rows, cols, np.float32, layout, what="dist2")              # (Roi knows u8 and f32: the words are read back as int32)
    c.mask_distance(mask_img, rows, cols, select, reach, d.img)
    c.synchronize()
    return d.result().view(np.int32)


def gpu_refine(c, mask_img, rows, cols, R, layout=(0, 0)):
    o = out_roi(rows, cols, np.uint8, layout, what="out")
    c.refine_mask(mask_img, rows, cols, MaskRefine(**R), o.img)
    c.synchronize()
    return o.result()


def check_plan(rows, cols, reach):
    p = mask_distance_plan(rows, cols, reach)
    assert p["path"] == ("lds" if reach <= L else "l2")
    assert p["bands"] == -(-rows // B) and p["blocks"] == -(-cols // W) and p["grid"] == (-(-cols // W), -(-rows // H))
    assert p["carry_words"] == -(-reach // B)
    return p


CASES = [(r, c, None) for r, c in SHAPES if r * c <= 20000] + [(r, c, m) for r, c in SHAPES if r * c > 20000 for m in MASKS]


@pytest.mark.parametrize("rows,cols,only", CASES, ids=lambda v: str(v))
def test_distance_bit_exact(ctx, rows, cols, only):
    """Every pair of mask, reach and select occurs (roi_util.covering) on every shape; the largest shape is split by mask."""
    combos = [cb for cb in covering(len(MASKS), len(REACHES), len(SELECTS)) if only is None or MASKS[cb[0]] == only]
    assert {cb[1] for cb in combos} == set(range(len(REACHES))) and {cb[2] for cb in combos} == {0, 1}
    paths, far, near = set(), 0, 0
    for mi, ri, si in combos:
        reach, select = REACHES[ri], SELECTS[si]
        paths.add(check_plan(rows, cols, reach)["path"])
        m, sel, E = case(MASKS[mi], rows, cols, select, reach)
        want = mr.distance(E, sel, reach)
        got = gpu_distance(ctx, up(m), rows, cols, select, reach)
        assert np.array_equal(got, want), (MASKS[mi], reach, select, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert (got != 0).all()
        far += int((np.abs(want) == mr.FAR).sum()); near += int((np.abs(want) != mr.FAR).sum())
    assert paths == {"lds", "l2"}
    if rows * cols > 1000 and only is None:
        assert far > 1000 and near > 1000                                    # both sides of the cut-off were met


def test_shapes_are_the_geometry_s():
    assert (H, W) in SHAPES and (H + 1, W + 1) in SHAPES and (B, 70) in SHAPES and (2 * B + 1, 70) in SHAPES and (9, W + 2 * L + 1) in SHAPES
    assert mask_distance_plan(2 * B + 1, 70, 65) == dict(path="lds", bands=3, blocks=2, carry_words=2, grid=(2, -(-(2 * B + 1) // H)),
                                                         words=2 * 3 * 70 + (2 * B + 1) * 70 + (2 * B + 1) * 2)
    assert L + 1 in REACHES and mask_distance_plan(9, W + 2 * L + 1, L + 1)["path"] == "l2"


@pytest.mark.parametrize("reach", [1, 2, 5, 13])
def test_a_single_pixel_gives_the_disc(ctx, reach):
    n = 2 * reach + 5
    m = mr.single_pixels(n, n, [(n // 2, n // 2)])
    got = gpu_distance(ctx, up(m), n, n, 0, reach)
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    r2 = yy * yy + xx * xx
    want = np.where(r2 == 0, -1, np.where(r2 <= reach * reach, r2, mr.FAR)).astype(np.int32)
    assert np.array_equal(got, want) and got[n // 2 - reach, n // 2 - reach] == mr.FAR


# every op, thresholds at k^2 and k^2 +- 1 for k of 1, 5, 64, both sides of the outline
THRESHOLDS = [1, 2, 24, 25, 26, 4095, 4096, 4097]
REFINES = ([dict(op=mr.GROW, outer2=t) for t in THRESHOLDS] + [dict(op=mr.SHRINK, inner2=t) for t in THRESHOLDS] +
           [dict(op=mr.OUTLINE, inner2=t) for t in THRESHOLDS] + [dict(op=mr.OUTLINE, outer2=t) for t in THRESHOLDS] +
           [dict(op=mr.OUTLINE, inner2=a, outer2=b) for a, b in ((1, 1), (25, 2), (2, 26), (4097, 24), (24, 4095))])
REFINE_MASKS = ["edges", "random1", "disc", "allbut", "full", "empty", "random"]


@pytest.mark.parametrize("rows,cols", [(37, 53), (2 * B + 1, 70), (9, W + 2 * L + 1), (257, 513)], ids=lambda v: str(v))
def test_refine_every_op_bit_exact(ctx, rows, cols):
    changed = 0
    n = len(REFINE_MASKS)
    for mi, ri, si in [(k % n, ri, (ri + k) % 2) for ri in range(len(REFINES)) for k in (ri, ri + 3)]:       # every rule on two masks, one per select
        R = mr.refine(SELECTS[si], **REFINES[ri])
        reach = mr.reach_of(R)
        assert reach == rt.refine_reach(R["op"], R["inner2"], R["outer2"])
        m, sel, E = case(REFINE_MASKS[mi], rows, cols, SELECTS[si], reach)
        want = mr.refine_mask(E, sel, R)
        got = gpu_refine(ctx, up(m), rows, cols, R)
        assert np.array_equal(got, want), (REFINE_MASKS[mi], R, int((got != want).sum()))
        changed += int(((want != 0) != sel).sum())
    assert changed > 100


@pytest.mark.parametrize("rows,cols", [(37, 53), (2 * B + 1, 70), (9, W + 2 * L + 1)], ids=lambda v: str(v))
def test_feather_grid_bit_exact(ctx, rows, cols):
    soft = 0
    pairs = [(lo, hi) for lo in LOHI for hi in LOHI if lo < hi]
    for i, (lo, hi) in enumerate(pairs):
        select = SELECTS[i % 2]
        R = mr.refine(select, mr.FEATHER, lo=lo, hi=hi)
        assert mr.reach_of(R) == rt.refine_reach(mr.FEATHER, lo=R["lo"], hi=R["hi"])
        for name in ("disc", "random1"):
            m, sel, E = case(name, rows, cols, select, 0)
            want = mr.refine_mask(E, sel, R)
            got = gpu_refine(ctx, up(m), rows, cols, R)
            assert np.array_equal(got, want), (name, R, int((got != want).sum()))
            soft += int(((want != 0) & (want != 255)).sum())
    for name in ("full", "empty"):                                          # E infinite: 255 inside, 0 outside
        m, sel, E = case(name, rows, cols, 0, 0)
        assert (gpu_refine(ctx, up(m), rows, cols, mr.refine(0, mr.FEATHER, lo=-3.0, hi=0.0)) == (255 if name == "full" else 0)).all()
    assert soft > 100


@pytest.mark.parametrize("rows,cols", [(37, 53), (130, 200)], ids=lambda v: str(v))
def test_distance_then_the_rule_is_refine(ctx, rows, cols):
    for select in SELECTS:
        m = case("disc", rows, cols, select, 0)[0]
        mi = up(m)
        for R in (mr.refine(select, mr.GROW, outer2=26), mr.refine(select, mr.SHRINK, inner2=24), mr.refine(select, mr.OUTLINE, inner2=1, outer2=4097),
                  mr.refine(select, mr.FEATHER, lo=-7.25, hi=0.5), mr.refine(select, mr.FEATHER, lo=-0.5, hi=1023.5)):
            d2 = gpu_distance(ctx, mi, rows, cols, select, mr.reach_of(R))
            assert np.array_equal(gpu_refine(ctx, mi, rows, cols, R), mr.refine_from_distance(d2, R)), R


def test_grow_is_remove_object_s_ring(ctx):
    """rtdd_remove_object with grow = 1 and every pixel eligible equals rtdd_remove_object with grow = 0 on the GROW outer2 = 2 mask."""
    rows, cols = 130, 200
    orig, depth = random_inputs(rows, cols, 77)
    o, d = up(orig), up(depth)
    for name, select in (("disc", CODE), ("random1", 0), ("edges", CODE)):
        m = case(name, rows, cols, select, 5)[0]
        mi, grown = up(m), up(np.zeros((rows, cols), np.uint8))
        ctx.refine_mask(mi, rows, cols, MaskRefine(select, REFINE_GROW, 0, 2), grown)
        outs = []
        for mask_img, R in ((mi, rt.Removal(select, 1, 0.0)), (grown, rt.Removal(0, 0, 0.0))):
            art, z = up(np.full((rows, cols, 3), FILL, np.uint8)), up(np.full((rows, cols), -7.0, np.float32))
            ctx.remove_object(o, d, mask_img, art, z, rows, cols, R)
            ctx.synchronize()
            outs.append((down(art), down(z)))
        assert_same_image(outs[0][0], outs[1][0], name)
        assert same_bits(outs[0][1], outs[1][1]) and not np.array_equal(outs[0][0], orig)


@pytest.mark.parametrize("rows,cols", [(37, 53), (130, 300)], ids=lambda v: str(v))
def test_matte_lift(ctx, rows, cols):
    orig, depth = random_inputs(rows, cols, rows)
    rng = np.random.default_rng(cols)
    alpha = rng.integers(0, 256, (rows, cols), dtype=np.uint8); alpha[rng.random((rows, cols)) < 0.3] = 0; alpha[rng.random((rows, cols)) < 0.3] = 255
    hard = np.where(alpha >= 128, 255, 0).astype(np.uint8)
    o, d, a, h = up(orig), up(depth), up(alpha), up(hard)
    sr, sc = 21, 30
    boxes = [(5, 4), (-sc // 2, 6), (cols - sc // 2, 6), (7, -sr // 2), (7, rows - sr // 2), (cols, 3), (3, rows + 1), (-40 * sc, 3)]
    for x, y in boxes:
        s, s0, s1 = (up(np.full((sr, sc, 4), FILL, np.uint8)) for _ in range(3))
        ctx.lift_layer_matte(o, a, rows, cols, x, y, s, sr, sc)
        ctx.lift_layer_matte(o, h, rows, cols, x, y, s0, sr, sc)
        ctx.lift_layer(o, h, rows, cols, 0, x, y, s1, sr, sc)
        ctx.synchronize()
        assert np.array_equal(down(s), mr.lift_matte(orig, alpha, x, y, sr, sc)), (x, y)
        assert np.array_equal(down(s0), down(s1)) and np.array_equal(down(s1), lift(orig, hard, 0, x, y, sr, sc))
    # composited back where it came from: the original, for any alpha
    big_r, big_c = rows + 9, cols + 300                                      # wider than a wave's span, the image inside it
    s, back = up(np.full((big_r, big_c, 4), FILL, np.uint8)), up(np.zeros_like(orig))
    ctx.lift_layer_matte(o, a, rows, cols, -150, -4, s, big_r, big_c)
    ctx.composite_layer(o, d, s, back, None, rows, cols, rt.Layer(**layer(big_r, big_c, -150, -4, 256, NEAREST, 255)))
    ctx.synchronize()
    assert np.array_equal(down(s), mr.lift_matte(orig, alpha, -150, -4, big_r, big_c))
    assert_same_image(down(back), orig, "matte lift composited back")


# (lead, pitch residue) indices of the mask, dist2 and out
@pytest.mark.parametrize("layout", [(0, 0, 0), (3, 0, 0), (0, 3, 0), (0, 0, 3), (5, 4, 6), (2, 6, 1), (4, 1, 2), (6, 5, 4), (1, 2, 5)],
                         ids=lambda v: "".join(map(str, v)))
def test_sub_image_views(ctx, layout):
    rows, cols = 37, 70
    m, sel, E = case("random", rows, cols, CODE, 0)
    lm, ld, lo = LAYOUTS_U8[layout[0]], LAYOUTS_F32[layout[1]], LAYOUTS_U8[layout[2]]
    mask = Roi(m, lm[0], pitch_for(cols, *lm), FILL_INPUT, what="mask")      # (0xFF around it: selected under select = 0 if ever read)
    for select in (0, CODE):
        s = mr.selected(m, select); Es = mr.e_scipy(s)
        for reach in (5, L + 1):
            assert np.array_equal(gpu_distance(ctx, mask.img, rows, cols, select, reach, ld), mr.distance(Es, s, reach))
        for R in (mr.refine(select, mr.GROW, outer2=5), mr.refine(select, mr.FEATHER, lo=-2.0, hi=1.0)):
            assert np.array_equal(gpu_refine(ctx, mask.img, rows, cols, R, lo), mr.refine_mask(Es, s, R))
    mask.assert_unchanged()
    orig = random_inputs(rows, cols, 3)[0]
    o = Roi(orig, lm[0], pitch_for(cols * 3, *lm), FILL_INPUT, what="original")
    sr, sc = 40, 61
    sp = Roi(np.zeros((sr, sc * 4), np.uint8), lo[0], pitch_for(sc * 4, *lo), FILL_OUTPUT, seed=7, what="sprite")
    ctx.lift_layer_matte(o.img, mask.img, rows, cols, -5, 10, sp.img, sr, sc)
    ctx.synchronize()
    assert np.array_equal(sp.result().reshape(sr, sc, 4), mr.lift_matte(orig, m, -5, 10, sr, sc))
    o.assert_unchanged(); mask.assert_unchanged()


def test_queued_behind_an_unsynchronised_estimate():
    """The mask is the estimate's own u8 depth map (byte != 0), read with no synchronisation since the estimate was queued."""
    bgr, ann, _ = load_pair("Dog")
    rows, cols = bgr.shape[:2]
    R = mr.refine(0, mr.SHRINK, inner2=9)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        estimate(c, bgr, ann)
        mask_img = c.pyramid_image(rt.IMG_DEPTH_U8, 0)[:2]
        out, d2 = up(np.zeros((rows, cols), np.uint8)), up(np.zeros((rows, cols), np.int32))
        c.refine_mask(mask_img, rows, cols, MaskRefine(**R), out)
        c.mask_distance(mask_img, rows, cols, 0, 16, d2)
        c.synchronize()
        m = c.pyramid_download(rt.IMG_DEPTH_U8, 0)
    sel = mr.selected(m, 0); E = mr.e_scipy(sel)
    assert sel.any() and not sel.all()
    assert np.array_equal(down(out), mr.refine_mask(E, sel, R)) and np.array_equal(down(d2), mr.distance(E, sel, 16))


def test_the_three_calls_are_replayed_after_a_healed_solve():
    rows, cols = 130, 200
    orig = random_inputs(rows, cols, 11)[0]
    m, sel, E = case("disc", rows, cols, CODE, 0)
    R = mr.refine(CODE, mr.FEATHER, lo=-3.0, hi=0.0)
    L15 = layer(rows, cols, 15, 0, 256, NEAREST, 255)                        # the object, moved 15 to the right
    kept = []

    def queue(c, o, d, arts):
        mi, a, d2 = up(m), up(np.full((rows, cols), FILL, np.uint8)), up(np.zeros((rows, cols), np.int32))
        s = up(np.full((rows, cols, 4), FILL, np.uint8))
        kept.append((a, d2, s))
        c.refine_mask(mi, rows, cols, MaskRefine(**R), a)
        c.mask_distance(mi, rows, cols, CODE, 7, d2)
        c.lift_layer_matte(o, a, rows, cols, 0, 0, s, rows, cols)
        c.composite_layer(o, d, s, arts[0], None, rows, cols, rt.Layer(**L15))

    solved, healed = clean_and_healed(queue, 1, orig)
    alpha = mr.refine_mask(E, sel, R)
    sprite = mr.lift_matte(orig, alpha, 0, 0, rows, cols)
    for a, d2, s in kept:
        assert np.array_equal(down(a), alpha) and np.array_equal(down(d2), mr.distance(E, sel, 7)) and np.array_equal(down(s), sprite)
    assert_same_image(healed[0], composite(orig, solved, sprite, L15)[0], "healed: the feathered object moved")
    assert ((alpha != 0) & (alpha != 255)).sum() > 100


def _raw(fn, base, override):
    a = dict(base); a.update(override)
    return fn(*a.values())


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 37, 53
    m = case("random", rows, cols, CODE, 0)[0]
    orig = random_inputs(rows, cols, 1)[0]
    p, z = C.c_void_p, C.c_size_t
    with rt.Context(0) as c:
        mi, o = up(m), up(orig)
        out, d2 = up(np.full((rows, cols), FILL, np.uint8)), up(np.full((rows, cols), 5, np.int32))
        s = up(np.full((9, 7, 4), FILL, np.uint8)).flatten(1)
        images = {"null context": dict(ctx=None), "null mask": dict(mask=None), "mask pitch short of a row": dict(maskPitch=z(cols - 1)),
                  "negative rows": dict(rows=-1), "negative cols": dict(cols=-1), "rows^2 + cols^2 >= 2^31": dict(rows=40000, cols=40000)}
        dist = dict(ctx=c._h, mask=p(mi.data_ptr()), maskPitch=z(mi.stride(0)), rows=rows, cols=cols, select=CODE, reach=5, dist2=p(d2.data_ptr()),
                    dist2Pitch=z(d2.stride(0) * 4))
        bad = dict(images, **{"null dist2": dict(dist2=None), "dist2 pitch short of a row": dict(dist2Pitch=z(cols * 4 - 4)),
                              "dist2 pitch no multiple of 4": dict(dist2Pitch=z(d2.stride(0) * 4 + 2)), "dist2 pointer off by 2": dict(dist2=p(d2.data_ptr() + 2)),
                              "dist2 == mask": dict(dist2=p(mi.data_ptr())), "select -1": dict(select=-1), "select 256": dict(select=256),
                              "reach 0": dict(reach=0), "reach 1025": dict(reach=1025)})
        for what, ov in bad.items():
            assert _raw(rt.lib().rtdd_mask_distance, dist, ov) == 1, what
        good = MaskRefine(CODE, REFINE_GROW, 0, 5)
        ref = dict(ctx=c._h, mask=p(mi.data_ptr()), maskPitch=z(mi.stride(0)), rows=rows, cols=cols, refine=C.byref(good), out=p(out.data_ptr()),
                   outPitch=z(out.stride(0)))
        bad = dict(images, **{"null out": dict(out=None), "out pitch short of a row": dict(outPitch=z(cols - 1)), "out == mask": dict(out=p(mi.data_ptr())),
                              "null refine": dict(refine=None)})
        for what, ov in bad.items():
            assert _raw(rt.lib().rtdd_refine_mask, ref, ov) == 1, what
        nan, inf, big = float("nan"), float("inf"), 1024 * 1024
        fields = [dict(select=-1), dict(select=256), dict(op=-1), dict(op=4), dict(op=REFINE_GROW, outer2=0), dict(op=REFINE_GROW, outer2=big + 1),
                  dict(op=REFINE_SHRINK, inner2=0), dict(op=REFINE_SHRINK, inner2=big + 1), dict(op=REFINE_OUTLINE, inner2=0, outer2=0),
                  dict(op=REFINE_OUTLINE, inner2=-1, outer2=4), dict(op=REFINE_OUTLINE, inner2=4, outer2=big + 1)]
        fields += [dict(op=REFINE_FEATHER, lo=lo, hi=hi) for lo, hi in ((0.0, 0.0), (1.0, -1.0), (-1024.0, 0.0), (0.0, 1024.0), (nan, 1.0), (0.0, nan), (-inf, 0.0), (0.0, inf))]
        for kw in fields:
            with pytest.raises(rt.RtddError) as e:
                c.refine_mask(mi, rows, cols, MaskRefine(**dict(dict(select=CODE, op=REFINE_GROW, inner2=3, outer2=5), **kw)), out)
            assert e.value.status == 1, kw
        matte = dict(ctx=c._h, original=p(o.data_ptr()), originalPitch=z(o.stride(0)), alpha=p(mi.data_ptr()), alphaPitch=z(mi.stride(0)), rows=rows, cols=cols,
                     x=2, y=3, sprite=p(s.data_ptr()), spritePitch=z(s.stride(0)), spriteRows=9, spriteCols=7)
        bad = {"null context": dict(ctx=None), "null original": dict(original=None), "null alpha": dict(alpha=None), "null sprite": dict(sprite=None),
               "original pitch short of a row": dict(originalPitch=z(cols * 3 - 1)), "alpha pitch short of a row": dict(alphaPitch=z(cols - 1)),
               "sprite pitch short of a row": dict(spritePitch=z(7 * 4 - 1)), "negative rows": dict(rows=-1), "negative cols": dict(cols=-1),
               "rows^2 + cols^2 >= 2^31": dict(rows=40000, cols=40000), "x low": dict(x=-16385), "x high": dict(x=16384), "y low": dict(y=-16385),
               "y high": dict(y=16384), "no sprite rows": dict(spriteRows=0), "no sprite cols": dict(spriteCols=0), "too many sprite rows": dict(spriteRows=16385),
               "too many sprite cols": dict(spriteCols=16385, spritePitch=z(1 << 20)), "in place": dict(sprite=p(o.data_ptr()))}
        for what, ov in bad.items():
            assert _raw(rt.lib().rtdd_lift_layer_matte, matte, ov) == 1, what
        c.synchronize()
        assert (down(out) == FILL).all() and (down(d2) == 5).all() and (down(s) == FILL).all()                 # nothing was launched
        # the limits themselves are accepted, and an empty image is nothing to do
        sel = mr.selected(m, CODE); E = mr.e_scipy(sel)
        for R in (mr.refine(CODE, mr.GROW, outer2=big), mr.refine(CODE, mr.OUTLINE, inner2=big), mr.refine(CODE, mr.FEATHER, lo=-1023.5, hi=1023.5)):
            c.refine_mask(mi, rows, cols, MaskRefine(**R), out)
            c.synchronize()
            assert np.array_equal(down(out), mr.refine_mask(E, sel, R)), R
        assert _raw(rt.lib().rtdd_mask_distance, dist, dict(rows=0)) == 0 and _raw(rt.lib().rtdd_refine_mask, ref, dict(cols=0)) == 0
        c.mask_distance(mi, rows, cols, 255, 1024, d2)
        c.synchronize()
        assert (down(d2) == mr.FAR).all()                                      # (no pixel carries 255: nothing is selected)
