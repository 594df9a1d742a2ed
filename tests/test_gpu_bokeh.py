"""The occlusion-aware lens blur (include/rtdd.h rtdd_simulate_bokeh) on the GPU (-m gpu): byte for byte against the numpy restatement of
tests/bokeh_ref.py, which knows nothing of the kernel -- windows wider than the image, ragged tiles, images smaller than a tile, both
sides of every halo class; bands of 1080p on the Dog depth map; the disc gather's bytes on a constant map, from the GPU itself; the
two-layer scene the effect exists for; the focus pixel read on the device behind an estimate; the heal log; FP contraction; padding bytes;
sub-image views; the host-side refusals; the harness.  No tolerance anywhere: everything behind the signed circle is integer."""
import ctypes as C
import functools

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from bokeh_ref import bokeh_by_offsets, signed_coc, two_layer_scene
from effect_gpu import ctx, dog_depth  # noqa: F401
from effect_gpu import (FILL, assert_bad_images_refused, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, padded_artistic,
                        harness_pair, pixel_form_behind_estimate, random_inputs, run_harness, tile_mirrored)
from gpu_util import down, up
from refocus_ref import kernel_size
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, pitch_for

pytestmark = pytest.mark.gpu


def aperture_for(rows, cols, K):
    """An aperture that gives the window scale K exactly."""
    a = (K + 0.5) / float(np.sqrt(np.float32(rows * rows + cols * cols)))
    assert kernel_size(rows, cols, a) == K
    return a


def _bokeh(c, o, d, rows, cols, aperture, f=0.0, at=None, align=512):
    """rtdd_simulate_bokeh into a fresh artistic image; at = (x, y): the pixel form.  Returns the image on the host."""
    art = up(np.full((rows, cols, 3), FILL, np.uint8), align)
    x, y = at if at is not None else (-1, -1)
    c.simulate_bokeh(o, d, art, rows, cols, aperture, f, x, y)
    c.synchronize()
    return down(art)


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols):
    return random_inputs(rows, cols, rows * 1000 + cols)


# 70 x 90 at K = 127: the window is wider than the image, ragged tiles both ways; 5 x 7, 1 x 300, 300 x 1: smaller than a tile;
# K = 17 / 19, 33 / 35, 64 .. 67: the last h of the halo classes 8, 16 and 32 and the first of the next; 130 x 150: a halo over several tiles
@pytest.mark.parametrize("shape,K,align", [((70, 90), 127, 1), ((5, 7), 127, 4), ((1, 300), 127, 1), ((300, 1), 127, 512),
                                           ((33, 200), 17, 1), ((33, 200), 19, 4), ((33, 200), 33, 512), ((33, 200), 35, 1),
                                           ((130, 150), 64, 4), ((130, 150), 65, 1), ((130, 150), 66, 512), ((40, 131), 126, 1)])
def test_random_inputs_bit_exact(ctx, shape, K, align):
    rows, cols = shape
    orig, depth = _inputs(rows, cols)
    o, d = up(orig, align), up(depth, align)
    a = aperture_for(rows, cols, K)
    for f in (100.0, 300.0):                                           # (300: clamped to 255, every circle in front of the focus)
        got = _bokeh(ctx, o, d, rows, cols, a, f, align=align)
        assert_same_image(got, bokeh_by_offsets(orig, depth, f, K), (shape, K, f))
        assert not np.array_equal(got, orig) or rows * cols == 1
    at = (cols // 3, rows - 1)
    got = _bokeh(ctx, o, d, rows, cols, a, at=at, align=align)
    assert_same_image(got, bokeh_by_offsets(orig, depth, float(depth[at[1], at[0]]), K), (shape, K, "pixel form"))


@pytest.mark.parametrize("K", [0, 1])
def test_window_scales_0_and_1_return_the_original(ctx, K):
    rows, cols = 70, 90
    orig, depth = _inputs(rows, cols)
    got = _bokeh(ctx, up(orig), up(depth), rows, cols, aperture_for(rows, cols, K), 100.0)
    assert_same_image(got, orig, K)


def test_a_map_with_a_nan_at_the_focus_pixel_focuses_at_zero(ctx):
    rows, cols = 33, 200
    orig, depth = _inputs(rows, cols)
    ys, xs = np.nonzero(np.isnan(depth))
    at = (int(xs[0]), int(ys[0]))
    a = aperture_for(rows, cols, 33)
    assert_same_image(_bokeh(ctx, up(orig), up(depth), rows, cols, a, at=at), bokeh_by_offsets(orig, depth, 0.0, 33), "NaN focus")


def test_1080p_bands_on_the_dog_map(ctx, dog_depth):
    """The default aperture (K = 55) at 1080p: the top 32 rows, 32 rows across a tile seam in the middle, the bottom 32 rows, and a band
    with the focus at a clicked pixel."""
    rows, cols = 1080, 1920
    orig = np.random.default_rng(rows).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = tile_mirrored(dog_depth, rows, cols)
    K = kernel_size(rows, cols, 0.025)
    assert K == 55
    o, d = up(orig), up(depth)
    f = float(np.median(depth))
    got = _bokeh(ctx, o, d, rows, cols, 0.025, f)
    s = signed_coc(depth, f, K)
    assert (s < -1).any() and (s > 1).any()
    for band in ((0, 32), (520, 552), (rows - 32, rows)):              # (528 = 33 * 16: a tile seam)
        assert_same_image(got[band[0]:band[1]], bokeh_by_offsets(orig, depth, f, K, band), band)
    at = (700, 300)
    got = _bokeh(ctx, o, d, rows, cols, 0.025, at=at)
    assert_same_image(got[280:312], bokeh_by_offsets(orig, depth, float(depth[at[1], at[0]]), K, (280, 312)), "pixel form")


@pytest.mark.parametrize("K", [55, 127])
def test_constant_map_gives_the_disc_gathers_bytes(ctx, K):
    rows, cols = 200, 300
    orig = _inputs(rows, cols)[0]
    o, d = up(orig), up(np.full((rows, cols), 180.0, np.float32))
    a = aperture_for(rows, cols, K)
    for f in (20.0, 255.0):                                            # behind the focus, in front of it
        art = up(np.zeros_like(orig))
        ctx.simulate_lens_blur(o, d, art, rows, cols, a, f, -1, -1, rt.APERTURE_DISC)
        ctx.synchronize()
        disc = down(art)
        assert not np.array_equal(disc, orig)
        assert_same_image(_bokeh(ctx, o, d, rows, cols, a, f), disc, (K, f))


def test_two_layer_scene(ctx):
    orig, depth, sq, K = two_layer_scene()
    rows, cols = depth.shape
    o, d = up(orig), up(depth)
    a = aperture_for(rows, cols, K)
    out = _bokeh(ctx, o, d, rows, cols, a, 10.0)                       # focus on the square: no halo
    assert np.array_equal(out[sq], orig[sq]) and (out[~sq][:, 2] == 0).all()
    art = up(np.zeros_like(orig))
    ctx.simulate_lens_blur(o, d, art, rows, cols, a, 10.0, -1, -1, rt.APERTURE_DISC)
    ctx.synchronize()
    assert (down(art)[~sq][:, 2] > 0).any()                            # ... which the disc gather has
    out = _bokeh(ctx, o, d, rows, cols, a, 200.0)                      # focus on the background: the square spills over it
    assert int((out[~sq][:, 2] > 0).sum()) == 2228
    assert_same_image(out, bokeh_by_offsets(orig, depth, 200.0, K), "focus 200")


def test_pixel_form_reads_the_map_behind_an_unsynchronised_estimate():
    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        if value is None:
            c.simulate_bokeh(o, d, art, rows, cols, 0.025, 0.0, x, y)
        else:
            c.simulate_bokeh(o, d, art, rows, cols, 0.025, value, -1, -1)

    bgr, depth, x, y, fv, image = pixel_form_behind_estimate(call)
    assert not np.array_equal(image, bgr)
    rows, cols = depth.shape
    band = (max(y - 16, 0), min(y + 16, rows))
    assert_same_image(image[band[0]:band[1]], bokeh_by_offsets(bgr, depth, fv, kernel_size(rows, cols, 0.025), band), "pixel form")


def test_bokeh_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = random_inputs(rows, cols, 2)[0]

    def queue(c, o, d, arts):
        c.simulate_bokeh(o, d, arts[0], rows, cols, 0.025, 0.0, 100, 200)
        c.simulate_bokeh(o, d, arts[1], rows, cols, 0.1, 128.0, -1, -1)

    solved, healed = clean_and_healed(queue, 2, orig)
    band = (184, 216)
    want = bokeh_by_offsets(orig, solved, float(solved[200, 100]), kernel_size(rows, cols, 0.025), band)
    assert_same_image(healed[0][band[0]:band[1]], want, "healed, pixel form")
    assert not np.array_equal(healed[0], orig) and not np.array_equal(healed[1], orig)


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 40, 500
    orig, depth = _inputs(rows, cols)
    o, d = up(orig), up(depth)
    a = aperture_for(rows, cols, 45)
    try:
        outs = []
        for contract in (0, 1):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            outs.append(_bokeh(ctx, o, d, rows, cols, a, 77.0))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    assert np.array_equal(outs[0], outs[1])
    assert_same_image(outs[0], bokeh_by_offsets(orig, depth, 77.0, 45), "contraction")


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 19, cols * 3 + 13
    orig, depth = _inputs(rows, cols)
    o, d = up(orig), up(depth)
    for K in (1, 21, 127):
        base, art = padded_artistic(rows, cols, pitch)
        ctx.simulate_bokeh(o, d, art, rows, cols, aperture_for(rows, cols, K), 128.0, -1, -1)
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert_same_image(down(art), bokeh_by_offsets(orig, depth, 128.0, K), (cols, K))


# (lead, pitch residue) of the original, the depth map and the artistic image: the aligned layout, and the unaligned leads
@pytest.mark.parametrize("layout", [(0, 0, 0), (3, 3, 2)], ids=["aligned", "unaligned leads"])
def test_sub_image_views(ctx, layout):
    rows, cols, K = 13, 131, 23
    orig, depth = _inputs(rows, cols)
    (lo, ro), (ld, rd), (la, ra) = LAYOUTS_U8[layout[0]], LAYOUTS_F32[layout[1]], LAYOUTS_U8[layout[2]]
    if layout[0]:
        assert lo % 4 and ld % 16 and la % 4
    o = Roi(orig, lo, pitch_for(cols * 3, lo, ro), FILL_INPUT, what="original")
    d = Roi(depth, ld, pitch_for(cols * 4, ld, rd), FILL_INPUT, what="depth")
    out = Roi(np.zeros_like(orig), la, pitch_for(cols * 3, la, ra), FILL_OUTPUT, seed=5, what="artistic")
    ctx.simulate_bokeh(o.img, d.img, out.img, rows, cols, aperture_for(rows, cols, K), 60.0, -1, -1)
    ctx.synchronize()
    assert_same_image(out.result(), bokeh_by_offsets(orig, depth, 60.0, K), layout)
    o.assert_unchanged(); d.assert_unchanged()


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = _inputs(rows, cols)
    sentinel = np.full_like(orig, 77)
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        bad = [dict(aperture=-0.01), dict(aperture=float("nan")), dict(aperture=float("inf")), dict(aperture=aperture_for(rows, cols, 128)),
               dict(aperture=aperture_for(rows, cols, 255)), dict(f=float("nan")), dict(f=float("inf")),
               dict(at=(cols, 0)), dict(at=(0, rows)), dict(at=(5, -1))]
        for kw in bad:
            x, y = kw.get("at", (-1, -1))
            with pytest.raises(rt.RtddError) as e:
                c.simulate_bokeh(o, d, art, rows, cols, kw.get("aperture", 0.025), kw.get("f", 0.0), x, y)
            assert e.value.status == 1, kw
        with pytest.raises(rt.RtddError) as e:
            c.simulate_bokeh(o, d, o, rows, cols, 0.025, 0.0, -1, -1)          # in place
        assert e.value.status == 1
        assert_bad_images_refused(c, rt.lib().rtdd_simulate_bokeh, o, d, art, rows, cols, (C.c_double(0.025), C.c_float(0.0), -1, -1))
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                            # nothing was launched
        # the limits themselves are accepted
        c.simulate_bokeh(o, d, art, rows, cols, aperture_for(rows, cols, 127), 0.0, cols - 1, rows - 1)
        c.simulate_bokeh(o, d, art, rows, cols, 0.0, -1e30, -1, 12345)
        c.synchronize()
        assert_same_image(down(art), orig, "K = 0")


def test_harness_bokeh_spread(tmp_path):
    bgr, ann = harness_pair(tmp_path, "pnm")
    rows, cols = bgr.shape[:2]
    spread = run_harness(tmp_path, "pnm", ["--effect", "refocus", "--focus-at", "300,200", "--bokeh", "spread"])[1]
    with rt.Context(0) as c:                                                  # the harness's own depth map: the same estimate
        c.GPULoadWeights(0.4)
        d = estimate(c, bgr, ann)
        o, a1, a2 = up(bgr), up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        c.simulate_bokeh(o, d, a1, rows, cols, 0.025, 0.0, 300, 200)
        c.simulate_lens_blur(o, d, a2, rows, cols, 0.025, 0.0, 300, 200, rt.APERTURE_DISC)
        c.synchronize()
        assert_same_image(spread, down(a1), "harness")
        assert not np.array_equal(spread, down(a2)) and not np.array_equal(spread, bgr)
