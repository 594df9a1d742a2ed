"""The round-aperture lens blur (include/rtdd.h rtdd_simulate_lens_blur) on the GPU (-m gpu): bit for bit against the restatements of
tests/lens_blur_ref.py on both paths (per-tile row prefixes in LDS, a global row-prefix table), at every size up to 8K; the square aperture
against rtdd_simulate_refocus; out-of-range depths; the table buffer shared with the defocus; the focus pixel read on the device behind
an estimate; the heal log; the host-side refusals; the dataset; the harness."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from dataset_util import PAIRS, load_pair
from effect_gpu import ctx  # noqa: F401
from effect_gpu import (assert_bad_images_refused, assert_same_image, clean_and_healed, estimate, harness_bin, harness_pair,
                        pixel_form_behind_estimate, run_harness)
from effects_ref import defocus_by_summed_area_table, effect_inputs
from gpu_util import down, up
from lens_blur_ref import lens_blur_by_row_prefixes, lens_blur_literal
from refocus_ref import kernel_size, largest_aperture

pytestmark = pytest.mark.gpu
FOCI = [0.0, 37.5, 128.0, 255.0]


def _blur(c, o, d, rows, cols, aperture=0.025, f=0.0, at=None, path=0, shape=rt.APERTURE_DISC):
    """rtdd_simulate_lens_blur into a fresh artistic image; at = (x, y): the pixel form.  Returns the image on the host."""
    art = up(np.zeros((rows, cols, 3), np.uint8))
    c.set_option(rt.OPT_DEFOCUS_PATH, path)
    try:
        x, y = at if at is not None else (-1, -1)
        c.simulate_lens_blur(o, d, art, rows, cols, aperture, f, x, y, shape)
        c.synchronize()
    finally:
        c.set_option(rt.OPT_DEFOCUS_PATH, 0)
    return down(art)


def _refocus(c, o, d, rows, cols, aperture=0.025, f=0.0, at=None, path=0):
    art = up(np.zeros((rows, cols, 3), np.uint8))
    c.set_option(rt.OPT_DEFOCUS_PATH, path)
    try:
        x, y = at if at is not None else (-1, -1)
        c.simulate_refocus(o, d, art, rows, cols, aperture, f, x, y)
        c.synchronize()
    finally:
        c.set_option(rt.OPT_DEFOCUS_PATH, 0)
    return down(art)


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols, seed):
    return effect_inputs(rows, cols, seed)


@functools.lru_cache(maxsize=None)
def _want(rows, cols, seed, f, aperture):
    """Restatement 2 of effect_inputs(rows, cols, seed) -- minutes of numpy at the large sizes, shared by the tests that need it."""
    orig, depth = _inputs(rows, cols, seed)
    return lens_blur_by_row_prefixes(orig, depth, f, aperture)


SMALL = [((6, 8), 512), ((23, 37), 1), ((67, 121), 1), ((131, 259), 4), ((270, 480), 512)]


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("shape,align", SMALL)
def test_disc_small_shapes_bit_exact(ctx, shape, align, path):
    rows, cols = shape
    orig, depth = effect_inputs(rows, cols, 31 + rows)
    o, d = up(orig, align), up(depth, align)
    at = (cols // 3, rows - 2)
    for aperture in (0.0, 0.01, 0.025, largest_aperture(rows, cols)):
        for f in FOCI + [None]:
            fv = float(depth[at[1], at[0]]) if f is None else f
            got = _blur(ctx, o, d, rows, cols, aperture, 0.0 if f is None else f, at=at if f is None else None, path=path)
            # (K = 255 never fits the tile region: both settings take the table there)
            assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == (2 if path == 2 and kernel_size(rows, cols, aperture) // 2 <= 28 else 1)
            want = lens_blur_by_row_prefixes(orig, depth, fv, aperture)
            assert_same_image(got, want, (aperture, f))
            if rows <= 67 and (aperture == 0.025 or f == 37.5):
                assert np.array_equal(got, lens_blur_literal(orig, depth, fv, aperture)), (aperture, f, "literal")


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("shape,align", SMALL)
def test_box_is_refocus_on_small_shapes(ctx, shape, align, path):
    rows, cols = shape
    orig, depth = effect_inputs(rows, cols, 31 + rows)
    o, d = up(orig, align), up(depth, align)
    at = (cols // 3, rows - 2)
    for aperture in (0.0, 0.025, largest_aperture(rows, cols)):
        for f in (0.0, 128.0):
            assert np.array_equal(_blur(ctx, o, d, rows, cols, aperture, f, path=path, shape=rt.APERTURE_BOX),
                                  _refocus(ctx, o, d, rows, cols, aperture, f, path=path)), (aperture, f)
        assert np.array_equal(_blur(ctx, o, d, rows, cols, aperture, at=at, path=path, shape=rt.APERTURE_BOX),
                              _refocus(ctx, o, d, rows, cols, aperture, at=at, path=path)), (aperture, "pixel")


@pytest.mark.parametrize("path", [0, 1])
def test_disc_1080p_every_pixel(ctx, path):
    """1080p: the tile kernel (automatic) and the table, every pixel; K = 255 does not fit the tile region -- the table takes it."""
    rows, cols = 1080, 1920
    orig, depth = _inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    got = _blur(ctx, o, d, rows, cols, f=128.0, path=path)
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == (2 if path == 0 else 1)
    want = _want(rows, cols, 9, 128.0, 0.025)
    assert_same_image(got, want, (path, "f = 128"))
    at = (1500, 900)
    got = _blur(ctx, o, d, rows, cols, at=at, path=path)
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == (2 if path == 0 else 1)
    want = _want(rows, cols, 9, float(depth[at[1], at[0]]), 0.025)
    assert_same_image(got, want, (path, "pixel form"))
    a = largest_aperture(rows, cols)
    got = _blur(ctx, o, d, rows, cols, a, 37.5, path=path)
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
    want = _want(rows, cols, 9, 37.5, a)
    assert_same_image(got, want, (path, "largest aperture"))


def test_box_is_refocus_at_1080p(ctx):
    rows, cols = 1080, 1920
    orig, depth = _inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    for path in (0, 1):
        for kw in (dict(f=128.0), dict(at=(1500, 900)), dict(aperture=largest_aperture(rows, cols), f=37.5)):
            assert np.array_equal(_blur(ctx, o, d, rows, cols, path=path, shape=rt.APERTURE_BOX, **kw), _refocus(ctx, o, d, rows, cols, path=path, **kw)), (path, kw)


def _smooth(rows, cols):
    from realtimedepthdiffusion_amd.synth import make_problem
    return np.ascontiguousarray(make_problem(rows, cols, seed=1)["gray"].astype(np.float32))


def test_disc_4k_every_pixel(ctx):
    rows, cols = 2160, 3840
    orig, depth = _inputs(rows, cols, 21)
    o = up(orig)
    got = _blur(ctx, o, up(depth), rows, cols, f=37.5)
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
    want = _want(rows, cols, 21, 37.5, 0.025)
    assert_same_image(got, want, "4K")
    smooth = _smooth(rows, cols)
    got = _blur(ctx, o, up(smooth), rows, cols, f=128.0)
    want = lens_blur_by_row_prefixes(orig, smooth, 128.0)
    assert_same_image(got, want, "4K, smooth map")


# 512 full-width rows of the 8K image: the first and the last 64, 128 across the middle, and four bands in between
BANDS_8K = [(0, 64), (1000, 1064), (2096, 2224), (3000, 3064), (3500, 3564), (4192, 4256), (4256, 4320)]


def test_disc_8k_bands(ctx):
    rows, cols = 4320, 7680
    assert sum(b - a for a, b in BANDS_8K) >= 512
    orig, depth = effect_inputs(rows, cols, 21)
    got = _blur(ctx, up(orig), up(depth), rows, cols, f=128.0)          # the whole image is rendered
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
    for band in BANDS_8K:
        want = lens_blur_by_row_prefixes(orig, depth, 128.0, band=band)
        assert_same_image(got[band[0]:band[1]], want, band)


def test_out_of_range_depths_are_clamped_and_nothing_sticks():
    rows, cols = 1080, 1920
    orig, depth = _inputs(rows, cols, 9)
    wild = depth.copy()
    for i, v in enumerate((-5.0, 1e9, np.nan, np.inf, -np.inf, 700.0)):
        wild[7 + 9 * i::50, 3 + 5 * i::40] = np.float32(v)
    wild[0, 0] = np.float32(1e9); wild[-1, -1] = np.float32(np.inf); wild[0, -1] = np.float32(np.nan)
    with rt.Context(0) as c:
        o, w = up(orig), up(wild)
        want = lens_blur_by_row_prefixes(orig, wild, 20.0)
        for path, last in ((0, 2), (1, 1)):
            got = _blur(c, o, w, rows, cols, f=20.0, path=path)            # (returns RTDD_OK: anything else raises)
            assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == last
            assert_same_image(got, want, path)
        art = up(np.zeros_like(orig))
        c.GPUSimulateDefocus(o, up(np.clip(depth, 0, 255)), art, rows, cols)
        c.synchronize()
        assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 2                  # the automatic choice is still the tile kernel


def test_defocus_and_lens_blur_share_the_table_buffer():
    """Defocus (table path, 4K), lens blur (global path), defocus again, on one context: the lens blur's row prefixes overwrite what the
    defocus table keeps zero, and the second defocus lays its table out again."""
    rows, cols = 2160, 3840
    orig, depth = _inputs(rows, cols, 21)
    want_defocus = defocus_by_summed_area_table(orig, depth)
    with rt.Context(0) as c:
        o, d = up(orig), up(depth)
        a1, a2, a3 = (up(np.zeros_like(orig)) for _ in range(3))
        c.GPUSimulateDefocus(o, d, a1, rows, cols)
        assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
        c.simulate_lens_blur(o, d, a2, rows, cols, 0.025, 37.5, -1, -1, rt.APERTURE_DISC)
        assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
        c.GPUSimulateDefocus(o, d, a3, rows, cols)
        c.synchronize()
        assert np.array_equal(down(a1), want_defocus)
        assert np.array_equal(down(a3), want_defocus)
        want = _want(rows, cols, 21, 37.5, 0.025)
        assert_same_image(down(a2), want, "between the two defocus calls")


def test_pixel_form_reads_the_map_behind_an_unsynchronised_estimate():
    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        if value is None:
            c.simulate_lens_blur(o, d, art, rows, cols, 0.025, 0.0, x, y)
        else:
            c.simulate_lens_blur(o, d, art, rows, cols, 0.025, value, -1, -1)

    bgr, _, _, _, _, image = pixel_form_behind_estimate(call)
    assert not np.array_equal(image, bgr)


def test_lens_blur_is_replayed_after_a_healed_solve():
    """A solve with a (simulated) time-out status and two lens blurs (pixel form: tile kernel and global table) queued behind it: the
    synchronisation heals the solve and renders both again from the healed depth -- the images of a clean run."""
    rows, cols = 270, 480
    orig = effect_inputs(rows, cols, 2)[0]

    def queue(c, o, d, arts):
        c.simulate_lens_blur(o, d, arts[0], rows, cols, 0.025, 0.0, 100, 200)
        c.simulate_lens_blur(o, d, arts[1], rows, cols, 0.2, 0.0, 100, 200)

    solved, healed = clean_and_healed(queue, 2, orig)
    assert np.array_equal(healed[0], lens_blur_by_row_prefixes(orig, solved, float(solved[200, 100])))


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = effect_inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        big = 256.5 / float(np.sqrt(np.float32(rows * rows + cols * cols)))
        assert kernel_size(rows, cols, big) == 256
        bad = [dict(aperture=-0.01), dict(aperture=float("nan")), dict(aperture=float("inf")), dict(aperture=big),
               dict(f=float("nan")), dict(f=float("inf")), dict(f=-float("inf")),
               dict(at=(cols, 0)), dict(at=(0, rows)), dict(at=(5, -1)), dict(at=(cols + 1000, rows + 1000)),
               dict(shape=2), dict(shape=-1), dict(shape=1000)]
        for kw in bad:
            x, y = kw.get("at", (-1, -1))
            for shape in ([kw["shape"]] if "shape" in kw else [rt.APERTURE_DISC, rt.APERTURE_BOX]):
                with pytest.raises(rt.RtddError) as e:
                    c.simulate_lens_blur(o, d, art, rows, cols, kw.get("aperture", 0.025), kw.get("f", 0.0), x, y, shape)
                assert e.value.status == 1, kw
        for shape in (rt.APERTURE_DISC, rt.APERTURE_BOX):
            with pytest.raises(rt.RtddError) as e:
                c.simulate_lens_blur(o, d, o, rows, cols, 0.025, 0.0, -1, -1, shape)      # in place
            assert e.value.status == 1
        for shape in (rt.APERTURE_DISC, rt.APERTURE_BOX):
            assert_bad_images_refused(c, rt.lib().rtdd_simulate_lens_blur, o, d, art, rows, cols, (C.c_double(0.025), C.c_float(0.0), -1, -1, shape))
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                            # nothing was launched
        # the limits themselves are accepted
        c.simulate_lens_blur(o, d, art, rows, cols, largest_aperture(rows, cols), 0.0, cols - 1, rows - 1)
        c.simulate_lens_blur(o, d, art, rows, cols, 0.0, -1e30, -1, 12345)
        c.synchronize()


@pytest.mark.parametrize("name", PAIRS)
def test_disc_at_the_clicked_pixel_on_the_dataset(name):
    """Every bundled pair at its own size: the estimate, then the disc focused on a pixel of the map."""
    bgr, ann, _ = load_pair(name)
    rows, cols = bgr.shape[:2]
    x, y = (2 * cols) // 5, (3 * rows) // 5
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = estimate(c, bgr, ann)
        o, art = up(bgr), up(np.zeros_like(bgr))
        c.simulate_lens_blur(o, d, art, rows, cols, 0.025, 0.0, x, y)
        c.synchronize()
        assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 2
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        got = down(art)
    want = lens_blur_by_row_prefixes(bgr, depth, float(depth[y, x]))
    assert_same_image(got, want, name)


def test_harness_bokeh(tmp_path):
    bgr, ann = harness_pair(tmp_path, "pnm")
    rows, cols = bgr.shape[:2]
    disc = run_harness(tmp_path, "pnm", ["--effect", "refocus", "--bokeh", "disc", "--focus-at", "300,200"])[1]
    box = run_harness(tmp_path, "pnm", ["--effect", "refocus", "--bokeh", "box", "--focus-at", "300,200"])[1]
    plain = run_harness(tmp_path, "pnm", ["--effect", "refocus", "--focus-at", "300,200"])[1]
    assert np.array_equal(box, plain)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = estimate(c, bgr, ann)
        o, a1, a2 = up(bgr), up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        c.simulate_lens_blur(o, d, a1, rows, cols, 0.025, 0.0, 300, 200, rt.APERTURE_DISC)
        c.simulate_refocus(o, d, a2, rows, cols, 0.025, 0.0, 300, 200)
        c.synchronize()
        assert np.array_equal(disc, down(a1))
        assert np.array_equal(box, down(a2))
    assert not np.array_equal(disc, box)


def test_harness_refuses_live_with_the_disc():
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3", "--effect", "refocus", "--bokeh", "disc"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--effect", "refocus", "--bokeh", "hexagon"], capture_output=True, text=True)
    assert r.returncode != 0 and "--bokeh wants box or disc" in r.stdout
