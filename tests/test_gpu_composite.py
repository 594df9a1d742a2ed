"""The composited layer (include/rtdd.h rtdd_composite_layer) on the GPU (-m gpu): byte for byte, and on the depth bit for bit, against the
numpy restatement of tests/composite_ref.py, which knows nothing of the kernel (no footprint, no vector path).  Shapes: 37 x 53 with a
9 x 7 sprite (no row is aligned: one pixel per lane) and 130 x 200 with a 70 x 90 sprite (several workgroups, both sides of the
footprint test, four pixels per lane with a ragged end).  Every scale, filter, feather, opacity, plane form, position and sprite alpha
of the issue, pairwise; depth maps with values outside [0, 255] and NaN; sub-image views of every pointer; depthOut NULL; behind an
unsynchronised estimate; the heal log; the refusals; the chain into the effects that read the composite's depth map; the harness.  No
tolerance anywhere."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd import LAYER_BILINEAR, LAYER_NEAREST, Layer          # (absent without the feature: nothing here runs)
from bokeh_ref import bokeh_by_offsets
from composite_ref import BILINEAR, NEAREST, composite, layer, random_sprite, same_bits
from dataset_util import load_pair
from effect_gpu import ctx  # noqa: F401
from effect_gpu import (FILL, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, harness_bin, harness_pair, padded_artistic,
                        random_inputs, raw_images, run_harness, write_pnm)
from gpu_util import down, up
from refocus_ref import kernel_size, refocus_by_summed_area_table
from relight_ref import light
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from shadow_ref import relight_shadowed, shadow

pytestmark = pytest.mark.gpu

ZFILL = -7.0                                     # what a depthOut image holds before the call writes it
SHAPES = {"small": ((37, 53), (9, 7)), "large": ((130, 200), (70, 90))}         # (image rows, cols), (sprite rows, cols)
SCALES = [16, 100, 256, 700, 4096]
FEATHERS = [0.0, 0.5, 40.0]
OPACITIES = [0, 128, 255]
ALPHAS = [0, 255, "ramp", "random"]


def planes(rows, cols):
    """dd = 0, axis-aligned both ways, oblique."""
    return [(5, 5, 5, 5), (3, 0, cols - 4, 0), (0, rows - 2, 0, 1), (-9, 4, cols + 11, rows - 7)]


def positions(rows, cols, srows, scols):
    """(-5, -4); one straddling each of the four borders; wholly outside on each side; x = -16384."""
    return [(-5, -4), (-scols // 2, rows // 3), (cols - scols // 2, rows // 3), (cols // 3, -srows // 2), (cols // 3, rows - srows // 2),
            (-40 * scols, 3), (cols + 1, 3), (3, -40 * srows), (3, rows + 1), (-16384, 2)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    (rows, cols), (srows, scols) = SHAPES[name]
    orig, depth = random_inputs(rows, cols, rows * 1000 + cols)              # depths in [-20, 275], 3 % NaN
    assert np.isnan(depth).any() and (depth < 0).any() and (depth > 255).any()
    sprites = {a: random_sprite(srows, scols, 7 + i, a) for i, a in enumerate(ALPHAS)}
    return orig, depth, sprites


def _composite(c, o, d, s, rows, cols, L, with_depth=True):
    """rtdd_composite_layer into fresh outputs.  Returns (artistic, depthOut or None) on the host."""
    art = up(np.full((rows, cols, 3), FILL, np.uint8))
    z = up(np.full((rows, cols), ZFILL, np.float32)) if with_depth else None
    c.composite_layer(o, d, s, art, z, rows, cols, Layer(**L))
    c.synchronize()
    return down(art), (down(z) if with_depth else None)


def assert_same(got, want, what):
    assert_same_image(got[0], want[0], what)
    assert same_bits(got[1], want[1]), f"{what}: {int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())} depths differ"


@pytest.mark.parametrize("filt", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_parameters_bit_exact(ctx, name, filt):
    """Every pair of levels of scale, feather, opacity, plane, position and alpha occurs (roi_util.covering)."""
    (rows, cols), (srows, scols) = SHAPES[name]
    orig, depth, sprites = _inputs(name)
    o, d = up(orig), up(depth)
    dev = {a: up(s) for a, s in sprites.items()}
    P, Q = planes(rows, cols), positions(rows, cols, srows, scols)
    changed = won = lost_nan = 0
    for i, (si, fi, oi, pi, qi, ai) in enumerate(covering(len(SCALES), len(FEATHERS), len(OPACITIES), len(P), len(Q), len(ALPHAS))):
        x, y = Q[qi]
        L = layer(srows, scols, x, y, SCALES[si], filt, OPACITIES[oi], *P[pi], depth0=30.0 + 7 * (i % 9), depth1=250.0 - 11 * (i % 7), feather=FEATHERS[fi])
        want = composite(orig, depth, sprites[ALPHAS[ai]], L)
        got = _composite(ctx, o, d, dev[ALPHAS[ai]], rows, cols, L)
        assert_same(got, want, (name, L, ALPHAS[ai]))
        changed += int(not np.array_equal(want[0], orig))
        moved = want[1].view(np.uint32) != depth.view(np.uint32)
        won += int(moved.any())
        lost_nan += int((np.isnan(want[1]) & ~moved).any())
    assert changed > 10 and won > 10 and lost_nan > 10                      # layers were drawn, won depths, and lost to NaN ... which was copied


@pytest.mark.parametrize("name", list(SHAPES))
def test_identities_on_the_gpu(ctx, name):
    (rows, cols), (srows, scols) = SHAPES[name]
    orig, depth, sprites = _inputs(name)
    o, d, s = up(orig), up(depth), up(sprites["random"])
    kw = dict(x0=0, y0=0, x1=cols, y1=rows, depth0=20.0, depth1=240.0, feather=30.0)
    near = _composite(ctx, o, d, s, rows, cols, layer(srows, scols, 11, 5, 256, NEAREST, 200, **kw))
    assert_same(_composite(ctx, o, d, s, rows, cols, layer(srows, scols, 11, 5, 256, BILINEAR, 200, **kw)), near, "bilinear at 256")
    assert not np.array_equal(near[0], orig)
    got = _composite(ctx, o, d, s, rows, cols, layer(srows, scols, 11, 5, 700, BILINEAR, 0, **kw))
    assert_same(got, (orig, depth), "opacity 0")
    art, z = _composite(ctx, o, d, up(sprites[255]), rows, cols, layer(srows, scols, 11, 5, 256, NEAREST, 255))
    want = orig.copy(); want[5:5 + srows, 11:11 + scols] = sprites[255][..., :3]
    assert_same_image(art, want, "paste")
    assert (z[5:5 + srows, 11:11 + scols] == 0).all()


def test_depth_out_null_writes_nothing_but_artistic(ctx):
    (rows, cols), (srows, scols) = SHAPES["large"]
    orig, depth, sprites = _inputs("large")
    o, d, s = up(orig), up(depth), up(sprites["ramp"])
    L = layer(srows, scols, 60, 20, 300, BILINEAR, 220, 0, 0, cols, 0, 10.0, 200.0, 12.0)
    want = composite(orig, depth, sprites["ramp"], L)
    art, z = _composite(ctx, o, d, s, rows, cols, L, with_depth=False)
    assert z is None
    assert_same_image(art, want[0], "depthOut NULL")
    assert same_bits(down(d), depth) and np.array_equal(down(o), orig) and np.array_equal(down(s), sprites["ramp"])


@pytest.mark.parametrize("cols", [53, 200])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 21, cols * 3 + 13
    orig, depth = random_inputs(rows, cols, cols)
    sprite = random_sprite(9, 7, 3)
    o, d, s = up(orig), up(depth), up(sprite)
    for filt in (NEAREST, BILINEAR):
        L = layer(9, 7, cols - 20, 4, 700, filt, 255, depth0=100.0, depth1=100.0, feather=0.5)
        base, art = padded_artistic(rows, cols, pitch)
        zbase = up(np.full((rows, cols + 5), ZFILL, np.float32)); z = zbase[:, :cols]
        ctx.composite_layer(o, d, s, art, z, rows, cols, Layer(**L))
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert (down(zbase)[:, cols:] == ZFILL).all(), "depthOut padding written"
        assert_same((down(art), down(z)), composite(orig, depth, sprite, L), (cols, filt))


# (lead, pitch residue) indices of the original, the depth map, the sprite, the artistic image and depthOut: the aligned layout, each image
# unaligned on its own (the others aligned: every term of the launcher's alignment test), and all of them unaligned
@pytest.mark.parametrize("layout", [(0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 3, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 3, 0), (0, 0, 0, 0, 3), (3, 3, 5, 4, 6)],
                         ids=["aligned", "original", "depth", "sprite", "artistic", "depthOut", "all"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_sub_image_views(ctx, name, layout):
    (rows, cols), (srows, scols) = SHAPES[name]
    orig, depth, sprites = _inputs(name)
    sprite = sprites["random"]
    (lo, ro), (ld, rd), (ls, rs), (la, ra), (lz, rz) = (LAYOUTS_U8[layout[0]], LAYOUTS_F32[layout[1]], LAYOUTS_U8[layout[2]], LAYOUTS_U8[layout[3]],
                                                        LAYOUTS_F32[layout[4]])
    o = Roi(orig, lo, pitch_for(cols * 3, lo, ro), FILL_INPUT, what="original")
    d = Roi(depth, ld, pitch_for(cols * 4, ld, rd), FILL_INPUT, what="depth")
    s = Roi(sprite.reshape(srows, scols * 4), ls, pitch_for(scols * 4, ls, rs), FILL_INPUT, what="sprite")
    out = Roi(np.zeros_like(orig), la, pitch_for(cols * 3, la, ra), FILL_OUTPUT, seed=5, what="artistic")
    zout = Roi(np.zeros_like(depth), lz, pitch_for(cols * 4, lz, rz), FILL_OUTPUT, seed=6, what="depthOut")
    for filt, scale in ((NEAREST, 100), (BILINEAR, 700)):
        L = layer(srows, scols, -3, 6, scale, filt, 230, 0, 0, cols, rows, 40.0, 210.0, 40.0)
        ctx.composite_layer(o.img, d.img, s.img, out.img, zout.img, rows, cols, Layer(**L))
        ctx.synchronize()
        assert_same((out.result(), zout.result()), composite(orig, depth, sprite, L), (name, layout, filt))
        o.assert_unchanged(); d.assert_unchanged(); s.assert_unchanged()


def test_queued_behind_an_unsynchronised_estimate():
    bgr, ann, _ = load_pair("Dog")
    rows, cols = bgr.shape[:2]
    sprite = random_sprite(70, 90, 11, "ramp")
    L = layer(70, 90, -20, -10, 600, BILINEAR, 255, 0, 0, cols, rows, 20.0, 120.0, 20.0)     # over the far upper left corner of the map
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        o, s = up(bgr), up(sprite)
        art, z = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), np.float32))
        d = estimate(c, bgr, ann)
        c.composite_layer(o, d, s, art, z, rows, cols, Layer(**L))          # no synchronisation since the estimate was queued
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        want = composite(bgr, depth, sprite, L)
        assert_same((down(art), down(z)), want, "behind an estimate")
    assert not np.array_equal(want[0], bgr) and not same_bits(want[1], depth)


def test_composite_is_replayed_after_a_healed_solve():
    rows, cols = 130, 200
    orig = _inputs("large")[0]
    sprite = random_sprite(70, 90, 12, "random")
    L = layer(70, 90, 40, 30, 400, BILINEAR, 255, 0, 0, cols, 0, 0.0, 255.0, 10.0)
    zs = []

    def queue(c, o, d, arts):
        s, z = up(sprite), up(np.full((rows, cols), ZFILL, np.float32))
        zs.append((s, z))
        c.composite_layer(o, d, s, arts[0], z, rows, cols, Layer(**L))
        c.composite_layer(arts[0], z, s, arts[1], None, rows, cols, Layer(**dict(L, x=-20, filter=NEAREST)))     # a second layer on the first composite

    solved, healed = clean_and_healed(queue, 2, orig)
    first = composite(orig, solved, sprite, L)
    assert_same((healed[0], down(zs[1][1])), first, "healed")
    assert same_bits(down(zs[0][1]), first[1])
    assert_same_image(healed[1], composite(first[0], first[1], sprite, dict(L, x=-20, filter=NEAREST))[0], "healed, second layer")
    assert not np.array_equal(healed[0], orig)


def _raw_call(c, o, d, s, art, z, rows, cols, L, override):
    """rtdd_composite_layer through the raw ABI; override: {argument name: value}.  Returns the status."""
    po, op, pd, dp, pa, ap = raw_images(o, d, art)
    a = dict(ctx=c._h, original=po, originalPitch=op, depth=pd, depthPitch=dp, sprite=C.c_void_p(s.data_ptr()), spritePitch=C.c_size_t(s.stride(0)),
             artistic=pa, artisticPitch=ap, depthOut=C.c_void_p(z.data_ptr()), depthOutPitch=C.c_size_t(z.stride(0) * 4), rows=rows, cols=cols,
             layer=C.byref(L) if L is not None else None)
    a.update(override)
    return rt.lib().rtdd_composite_layer(*a.values())


def test_invalid_arguments_are_refused_on_the_host():
    (rows, cols), (srows, scols) = SHAPES["small"]
    orig, depth, sprites = _inputs("small")
    good = layer(srows, scols, 4, 3, 300, BILINEAR, 200, 0, 0, 10, 10, 20.0, 200.0, 5.0)
    with rt.Context(0) as c:
        o, d, s = up(orig), up(depth), up(sprites["random"])
        art, z = up(np.full_like(orig, FILL)), up(np.full((rows, cols), ZFILL, np.float32))
        po, op, pd, dp, pa, ap = raw_images(o, d, art)
        pz, zp = z.data_ptr(), z.stride(0) * 4
        images = {"null context": dict(ctx=None), "null original": dict(original=None), "null depth": dict(depth=None), "null artistic": dict(artistic=None),
                  "original pitch short of a row": dict(originalPitch=C.c_size_t(cols * 3 - 1)), "depth pitch short of a row": dict(depthPitch=C.c_size_t(cols * 4 - 4)),
                  "artistic pitch short of a row": dict(artisticPitch=C.c_size_t(cols * 3 - 1)), "depthOut pitch short of a row": dict(depthOutPitch=C.c_size_t(cols * 4 - 4)),
                  "depth pitch no multiple of 4": dict(depthPitch=C.c_size_t(dp.value + 2)), "depth pointer off by 2 bytes": dict(depth=C.c_void_p(pd.value + 2)),
                  "depthOut pitch no multiple of 4": dict(depthOutPitch=C.c_size_t(zp + 2)), "depthOut pointer off by 2 bytes": dict(depthOut=C.c_void_p(pz + 2)),
                  "negative rows": dict(rows=-1), "negative cols": dict(cols=-1), "rows^2 + cols^2 >= 2^31": dict(rows=40000, cols=40000),
                  "original == artistic": dict(artistic=po, artisticPitch=op), "depth == depthOut": dict(depthOut=pd, depthOutPitch=dp),
                  "null sprite": dict(sprite=None), "sprite pitch short of a row": dict(spritePitch=C.c_size_t(scols * 4 - 1)), "null layer": dict(layer=None)}
        for what, override in images.items():
            assert _raw_call(c, o, d, s, art, z, rows, cols, Layer(**good), override) == 1, what
        assert _raw_call(c, o, d, s, art, z, rows, cols, Layer(**good), dict(rows=0)) == 0                     # (the call itself is sound: an empty image)
        nan, inf = float("nan"), float("inf")
        fields = [dict(rows=0), dict(rows=16385), dict(cols=0), dict(cols=16385), dict(rows=-1), dict(x=-16385), dict(x=16384), dict(y=-16385), dict(y=16384),
                  dict(scale=15), dict(scale=4097), dict(scale=0), dict(scale=-256), dict(filter=2), dict(filter=-1), dict(opacity=-1), dict(opacity=256),
                  dict(x0=-16385), dict(x0=16384), dict(y0=-16385), dict(y0=16384), dict(x1=-16385), dict(x1=16384), dict(y1=-16385), dict(y1=16384),
                  dict(depth0=-0.5), dict(depth0=255.5), dict(depth0=nan), dict(depth0=inf), dict(depth1=-0.5), dict(depth1=255.5), dict(depth1=nan), dict(depth1=-inf),
                  dict(feather=-1.0), dict(feather=nan), dict(feather=inf)]
        for kw in fields:
            bad = dict(good, **kw)
            if bad["cols"] > scols or bad["rows"] > srows:                   # (a refusal by range, whatever the pitch: give the pitch room)
                assert _raw_call(c, o, d, s, art, z, rows, cols, Layer(**bad), dict(spritePitch=C.c_size_t(1 << 20))) == 1, kw
            else:
                with pytest.raises(rt.RtddError) as e:
                    c.composite_layer(o, d, s, art, z, rows, cols, Layer(**bad))
                assert e.value.status == 1, kw
        c.synchronize()
        assert (down(art) == FILL).all() and (down(z) == ZFILL).all()       # nothing was launched
        # the limits themselves are accepted
        for kw in (dict(x=-16384, y=16383, x0=-16384, y0=-16384, x1=16383, y1=16383, depth0=0.0, depth1=255.0, feather=0.0, opacity=0, scale=16),
                   dict(scale=4096, opacity=255, feather=1e30)):
            L = dict(good, **kw)
            c.composite_layer(o, d, s, art, z, rows, cols, Layer(**L))
            c.synchronize()
            assert_same((down(art), down(z)), composite(orig, depth, sprites["random"], L), kw)
        c.composite_layer(o, d, s, art, z, 0, cols, Layer(**good))           # an empty image: nothing to do
        big = up(np.zeros((1, 16384, 4), np.uint8))                          # the largest sprite width
        c.composite_layer(o, d, big, art, None, rows, cols, Layer(**dict(good, rows=1, cols=16384, scale=4096, x=-500)))
        c.synchronize()
        assert_same_image(down(art), orig, "a transparent sprite")


def test_chain_into_the_effects_that_read_the_depth_map(ctx):
    """composite, then rtdd_simulate_relight_shadowed and rtdd_simulate_bokeh on (artistic, depthOut): the restatements chained."""
    rows, cols = 60, 80
    rng = np.random.default_rng(9)
    orig = rng.integers(40, 256, (rows, cols, 3), dtype=np.uint8)
    depth = np.full((rows, cols), 200, np.float32); depth[10:50, 8:24] = 40; depth += rng.uniform(-3, 3, (rows, cols)).astype(np.float32)
    sprite = random_sprite(20, 30, 13, 255)
    L = layer(20, 30, 16, 20, 256, NEAREST, 255, depth0=120.0, depth1=120.0)
    o, d, s = up(orig), up(depth), up(sprite)
    art, z = up(np.zeros_like(orig)), up(np.zeros_like(depth))
    lit, blur = up(np.zeros_like(orig)), up(np.zeros_like(orig))
    Lt, S = light(x=-1.0, y=0.2, z=1.0, relief=0.1, ambient=0.2), shadow(maxSteps=64, bias=0.25)
    K = 21
    aperture = (K + 0.5) / float(np.sqrt(np.float32(rows * rows + cols * cols)))
    assert kernel_size(rows, cols, aperture) == K
    ctx.composite_layer(o, d, s, art, z, rows, cols, Layer(**L))
    ctx.simulate_relight_shadowed(art, z, lit, rows, cols, rt.Light(**Lt), rt.Shadow(**S))
    ctx.simulate_bokeh(art, z, blur, rows, cols, aperture, 120.0, -1, -1)
    ctx.synchronize()
    want = composite(orig, depth, sprite, L)
    assert_same((down(art), down(z)), want, "composite")
    assert (want[1] == 120).sum() == 20 * (30 - 8)                           # the sprite minus what the box hides
    assert_same_image(down(lit), relight_shadowed(want[0], want[1], Lt, S), "relight_shadowed on the composite")
    assert not np.array_equal(down(lit), relight_shadowed(want[0], depth, Lt, S))      # the depth map matters
    assert_same_image(down(blur), bokeh_by_offsets(want[0], want[1], 120.0, K), "bokeh on the composite")
    assert np.array_equal(down(blur)[25:35, 30:40], want[0][25:35, 30:40])              # the sprite is in focus at its own depth


def test_harness_layer_then_refocus(tmp_path):
    bgr, ann = harness_pair(tmp_path, "pnm")
    rows, cols = bgr.shape[:2]
    sprite = random_sprite(60, 80, 14, "ramp")
    write_pnm(tmp_path / "sprite.ppm", sprite[..., 2::-1]); write_pnm(tmp_path / "alpha.pgm", sprite[..., 3])        # (the file is RGB)
    args = ["--layer", str(tmp_path / "sprite.ppm"), "--layer-alpha", str(tmp_path / "alpha.pgm"), "--layer-at", "250,150", "--layer-scale", "384",
            "--layer-filter", "bilinear", "--layer-plane", "250,0,60,370,0,200", "--layer-feather", "8", "--layer-opacity", "240"]
    got = run_harness(tmp_path, "pnm", args + ["--effect", "refocus", "--focus", "128"])[1]
    L = layer(60, 80, 250, 150, 384, BILINEAR, 240, 250, 0, 370, 0, 60.0, 200.0, 8.0)
    with rt.Context(0) as c:                                                  # the harness's own depth map: the same estimate
        c.GPULoadWeights(0.4)
        estimate(c, bgr, ann)
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
    art, z = composite(bgr, depth, sprite, L)
    assert not np.array_equal(art, bgr) and not same_bits(z, depth)
    assert_same_image(got, refocus_by_summed_area_table(art, z, 128.0), "harness: layer, then refocus")
    assert not np.array_equal(got, refocus_by_summed_area_table(bgr, depth, 128.0))


def test_harness_refuses_live_with_a_layer(tmp_path):
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3", "--layer", "unused.ppm", "--layer-alpha", "unused.pgm", "--layer-at", "1,1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout
