"""Relighting with cast shadows (include/rtdd.h rtdd_simulate_relight_shadowed) on the GPU (-m gpu): bit for bit against the numpy
restatement of tests/shadow_ref.py, which knows nothing of the kernel -- small and odd shapes and alignments, both kinds of light, both
forms of the anchor, hard and soft shadows, 1 to 1024 steps, NaN and out-of-range depths, 1080p in full and bands of 4K and 8K; padding
bytes; FP contraction; the identities; the anchor pixel read on the device behind an estimate; the heal log; the host-side refusals; the
harness.  No tolerance anywhere: every operation of the header is a correctly rounded IEEE one."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from effect_gpu import ctx, dog_depth  # noqa: F401
from effect_gpu import (assert_bad_images_refused, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, harness_bin,
                        harness_files, harness_pair, padded_artistic, pixel_form_behind_estimate, random_inputs, run_harness, tile_mirrored)
from gpu_util import down, up
from relight_ref import DIRECTIONAL, POINT, apply_gain, light, relight, shade
from shadow_ref import relight_shadowed, shadow, shadow_q

pytestmark = pytest.mark.gpu
F = np.float32


def _run(c, o, d, rows, cols, L, S, align=512):
    art = up(np.zeros((rows, cols, 3), np.uint8), align)
    c.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**L), rt.Shadow(**S))
    c.synchronize()
    return down(art)


def _relight(c, o, d, rows, cols, L):
    art = up(np.zeros((rows, cols, 3), np.uint8))
    c.simulate_relight(o, d, art, rows, cols, rt.Light(**L))
    c.synchronize()
    return down(art)


def _lights(rows, cols, relief):
    """Directional lights along both major axes and a diagonal; point lights inside and outside the image, anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.125, diffuse=1.5)
    ax, ay = cols // 3, rows - 1
    return [light(DIRECTIONAL, -1, -1, 1, color=(255, 128, 7), **common),
            light(DIRECTIONAL, 3.5, -0.25, 0.5, **common),
            light(DIRECTIONAL, 0.3, 2, 0.015625, **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, -3000.5, rows + 7.25, 2000, anchorDepth=255, radius=5000, color=(10, 200, 255), **common),
            light(POINT, ax, ay, 0.5, anchorX=ax, anchorY=ay, radius=3, **common),
            light(POINT, cols + 40.0, 1.0, 25, anchorX=0, anchorY=0, radius=0.001, ambient=0.0, diffuse=8.0, relief=relief)]


def _shadows():
    return [shadow(1), shadow(7, bias=0.5, softness=0.75, strength=0.875), shadow(64, bias=2.0), shadow(1024, softness=3.0, strength=0.5),
            shadow(1024, bias=0.25)]


@pytest.mark.parametrize("shape,align", [((1, 1), 1), ((1, 37), 1), ((23, 1), 512), ((5, 255), 1), ((7, 257), 4), ((9, 1027), 1),
                                         ((3, 2051), 512), ((6, 1024), 512), ((5, 255), 4), ((9, 1027), 512)])
def test_small_shapes_bit_exact(ctx, shape, align):
    rows, cols = shape
    orig, depth = random_inputs(rows, cols, rows * 1000 + cols)
    o, d = up(orig, align), up(depth, align)
    for relief in (0.5, 64.0):
        for L in _lights(rows, cols, relief):
            for S in _shadows():
                assert_same_image(_run(ctx, o, d, rows, cols, L, S, align), relight_shadowed(orig, depth, L, S), (shape, align, L, S))


def test_tall_shapes_and_vertical_marches(ctx):
    """More rows than a workgroup holds, marches that cross many rows, a smooth map with long shadows."""
    rows, cols = 150, 203
    orig = random_inputs(rows, cols, 5)[0]
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    depth = (127.5 + 120 * np.sin(xx / 17.0) * np.cos(yy / 11.0)).astype(np.float32)
    o, d = up(orig, 1), up(depth, 1)
    shadowed = 0.0
    for L in _lights(rows, cols, 1.0) + [light(DIRECTIONAL, 0, 1, 0.25, relief=2), light(DIRECTIONAL, 0.5, -1, 2, relief=4)]:
        for S in (shadow(1024, bias=0.125), shadow(200, softness=0.5, strength=0.75)):
            assert_same_image(_run(ctx, o, d, rows, cols, L, S, 1), relight_shadowed(orig, depth, L, S), (L, S))
            shadowed = max(shadowed, float((shadow_q(depth, L, S) > 0).mean()))
    assert 0.2 < shadowed < 1.0


def test_out_of_range_and_non_finite_depths(ctx):
    rows, cols = 6, 300
    orig, depth = random_inputs(rows, cols, 21)
    depth[1, ::7] = np.inf; depth[2, ::5] = -np.inf; depth[3, ::3] = 1e30; depth[4, ::2] = -1e30; depth[5] = np.nan
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 2.0):
        for S in (shadow(64), shadow(64, bias=1.0, softness=1e-3), shadow(1024, softness=65536.0)):
            assert_same_image(_run(ctx, o, d, rows, cols, L, S), relight_shadowed(orig, depth, L, S), (L, S))


def test_extreme_parameters(ctx):
    """The bounds of the ranges; a direction whose m is tiny (an infinite rise: nothing is shadowed); a denormal softness."""
    rows, cols = 12, 140
    orig, depth = random_inputs(rows, cols, 23)
    o, d = up(orig), up(depth)
    cases = [(light(DIRECTIONAL, 1e-30, 0, 1, relief=64), shadow(1024)),
             (light(DIRECTIONAL, 1e-42, -1e-43, 1, relief=64), shadow(1024, softness=1e-40)),
             (light(DIRECTIONAL, -1, 0.5, 1e-30, relief=64), shadow(1024, bias=65536.0)),
             (light(DIRECTIONAL, -1, 0.5, 1e-30, relief=64), shadow(1024, bias=0.0, softness=1e-40, strength=1.0)),
             (light(DIRECTIONAL, 1, 1, 1e-6, relief=0.015625), shadow(1024, softness=65536.0)),
             (light(POINT, 32767, -32768, 65536, anchorDepth=0, radius=65536, relief=64), shadow(1024, softness=0.5)),
             (light(POINT, 70.0, 6.0, 1e-30, anchorDepth=255, radius=10, relief=64), shadow(1024, bias=1e-30))]
    for L, S in cases:
        assert_same_image(_run(ctx, o, d, rows, cols, L, S), relight_shadowed(orig, depth, L, S), (L, S))


def test_identities_on_the_device(ctx):
    rows, cols = 33, 700
    orig, depth = random_inputs(rows, cols, 22)
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 1.5):
        want = _relight(ctx, o, d, rows, cols, L)                       # rtdd_simulate_relight's own output
        assert_same_image(want, relight(orig, depth, L), "relight")
        for S in (shadow(0), shadow(0, bias=3, softness=2, strength=0.5), shadow(64, strength=0.0)):
            assert_same_image(_run(ctx, o, d, rows, cols, L, S), want, ("no shadow", L, S))
        if L["kind"] == DIRECTIONAL:
            assert not np.array_equal(_run(ctx, o, d, rows, cols, L, shadow(64)), want)
    # a light straight above: m == 0
    L = light(DIRECTIONAL, 0, 0, 3, relief=7, ambient=0.1, diffuse=1)
    assert_same_image(_run(ctx, o, d, rows, cols, L, shadow(1024)), _relight(ctx, o, d, rows, cols, L), "m == 0")
    # a constant map under lights that do not stand below it
    const = np.full((rows, cols), 93.5, np.float32)
    dc = up(const)
    for L in (light(DIRECTIONAL, -1, 0.25, 0.001, relief=64), light(POINT, 40.5, 2.5, 1e-3, anchorX=17, anchorY=3, radius=60, relief=64)):
        for S in (shadow(1024), shadow(1024, softness=1e-6)):
            assert_same_image(_run(ctx, o, dc, rows, cols, L, S), _relight(ctx, o, dc, rows, cols, L), ("constant", L, S))
    # mirror
    of, df = up(np.ascontiguousarray(orig[:, ::-1])), up(np.ascontiguousarray(depth[:, ::-1]))
    common = dict(relief=1.5, ambient=0.125, diffuse=1.0, color=(255, 200, 90))
    S = shadow(100, bias=0.5, softness=0.5, strength=0.75)
    a = _run(ctx, o, d, rows, cols, light(POINT, 40.5, 2.5, 30, anchorX=17, anchorY=3, radius=60, **common), S)
    b = _run(ctx, of, df, rows, cols, light(POINT, cols - 1 - 40.5, 2.5, 30, anchorX=cols - 1 - 17, anchorY=3, radius=60, **common), S)
    assert_same_image(b, a[:, ::-1], "mirror, point")
    a = _run(ctx, o, d, rows, cols, light(DIRECTIONAL, 1.25, -0.5, 0.75, **common), S)
    b = _run(ctx, of, df, rows, cols, light(DIRECTIONAL, -1.25, -0.5, 0.75, **common), S)
    assert_same_image(b, a[:, ::-1], "mirror, directional")


def test_known_answer_on_the_device(ctx):
    rows, cols = 2, 200
    depth = np.full((rows, cols), 255.0, np.float32)
    depth[:, :20] = 155.0
    orig = np.full((rows, cols, 3), 200, np.uint8)
    L = light(DIRECTIONAL, -1, 0, 1, relief=1, ambient=0.25, diffuse=1)
    o, d = up(orig), up(depth)
    lit = _relight(ctx, o, d, rows, cols, L)
    for steps, last in ((1024, 118), (50, 69)):
        out = _run(ctx, o, d, rows, cols, L, shadow(steps))
        assert (out[:, 20:last + 1] == 50).all() and np.array_equal(out[:, last + 1:], lit[:, last + 1:]) and np.array_equal(out[:, :20], lit[:, :20])


def _restate_rows(orig, depth, L, S, y0, y1, workers=16):
    """relight_shadowed(rows=(y0, y1)) with the marches of the rows shared out over threads: (image rows, share of pixels with q > 0)."""
    edges = np.linspace(y0, y1, min(workers, y1 - y0) + 1).astype(int)
    with ThreadPoolExecutor(workers) as ex:
        q = np.concatenate(list(ex.map(lambda ab: shadow_q(depth, L, S, (int(ab[0]), int(ab[1]))), zip(edges[:-1], edges[1:]))), 0)
    s = shade(depth, L)[y0:y1] * (F(1) - (F(S["strength"]) * q))
    assert s.dtype == F
    return apply_gain(orig[y0:y1], s, L), float((q > 0).mean())


# every pixel at 1080p; at 4K and 8K a band of 512 rows, whose rays leave it and are restated on the rows they reach
@pytest.mark.parametrize("rows,cols,band", [(1080, 1920, (0, 1080)), (2160, 3840, (900, 1412)), (4320, 7680, (3000, 3512))])
def test_full_size(ctx, dog_depth, rows, cols, band):
    rng = np.random.default_rng(rows)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = tile_mirrored(dog_depth, rows, cols)
    o, d = up(orig), up(depth)
    cases = [(light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1.0), shadow(256)),
             (light(POINT, cols * 0.4, rows * 0.3, 120, anchorX=cols // 2, anchorY=rows // 2, radius=cols / 4, relief=1.5, ambient=0.1, diffuse=3.0,
                    color=(200, 230, 255)), shadow(256, bias=0.5, softness=0.5, strength=0.875))]
    if rows == 1080:
        cases.append((light(DIRECTIONAL, 3.5, -0.25, 0.5, relief=2, ambient=0.25, diffuse=1.0), shadow(256, bias=1.0, softness=1.0)))
    y0, y1 = band
    for L, S in cases:
        pitch = cols * 3 + 512
        base, art = padded_artistic(rows, cols, pitch)
        ctx.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**L), rt.Shadow(**S))
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        want, share = _restate_rows(orig, depth, L, S, y0, y1)
        print(f"{rows} x {cols} rows {y0}-{y1} kind {L['kind']} softness {S['softness']}: {share:.3f} of the pixels shadowed")
        assert 0.0 < share < 1.0
        assert_same_image(down(art)[y0:y1], want, (rows, L["kind"], S))


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 5, cols * 3 + 13
    orig, depth = random_inputs(rows, cols, 8)
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 1.0)[1:5]:
        S = shadow(64, softness=0.5)
        base, art = padded_artistic(rows, cols, pitch)
        ctx.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**L), rt.Shadow(**S))
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert_same_image(down(art), relight_shadowed(orig, depth, L, S), L)


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 16, 1500
    orig, depth = random_inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 3.0):
        for S in (shadow(64, bias=0.5), shadow(64, softness=0.75, strength=0.5)):
            try:
                outs = []
                for contract in (0, 1):
                    ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                    outs.append(_run(ctx, o, d, rows, cols, L, S))
            finally:
                ctx.set_option(rt.OPT_FP_CONTRACT, 1)
            assert np.array_equal(outs[0], outs[1])
            assert_same_image(outs[0], relight_shadowed(orig, depth, L, S), "contraction")


def test_anchor_pixel_is_read_behind_an_unsynchronised_estimate():
    S = shadow(128, bias=0.5, softness=0.5)

    def over(x, y):
        return light(POINT, x, y, 60, anchorX=x, anchorY=y, radius=150, relief=2, ambient=0.2, diffuse=2.0)

    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        L = over(x, y) if value is None else dict(over(x, y), anchorX=-1, anchorY=-1, anchorDepth=value)
        c.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**L), rt.Shadow(**S))

    bgr, depth, x, y, _, image = pixel_form_behind_estimate(call)
    assert_same_image(image, relight_shadowed(bgr, depth, over(x, y), S), "pixel form")
    assert not np.array_equal(image, relight(bgr, depth, over(x, y)))


def test_shadowed_relight_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = random_inputs(rows, cols, 2)[0]
    L1 = light(POINT, 100, 200, 40, anchorX=100, anchorY=200, radius=120, relief=2, ambient=0.2, diffuse=2.0, color=(255, 220, 180))
    L2 = light(DIRECTIONAL, 1, -2, 1.5, relief=3, ambient=0.1, diffuse=1.25)
    S1, S2 = shadow(96, bias=0.5, softness=0.5, strength=0.875), shadow(200)

    def queue(c, o, d, arts):
        light1, shadow1 = rt.Light(**L1), rt.Shadow(**S1)
        c.simulate_relight_shadowed(o, d, arts[0], rows, cols, light1, shadow1)
        light1.kind, light1.relief, light1.x = 7, -1.0, float("nan")   # the call has read both: the record holds them by value
        shadow1.maxSteps, shadow1.bias, shadow1.strength = -5, float("nan"), 9.0
        c.simulate_relight_shadowed(o, d, arts[1], rows, cols, rt.Light(**L2), rt.Shadow(**S2))

    solved, healed = clean_and_healed(queue, 2, orig)
    assert_same_image(healed[0], relight_shadowed(orig, solved, L1, S1), "healed point light")
    assert_same_image(healed[1], relight_shadowed(orig, solved, L2, S2), "healed directional light")
    assert not np.array_equal(healed[1], relight(orig, solved, L2))


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = random_inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    nan, inf = float("nan"), float("inf")
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        pt = dict(kind=POINT, x=10.0, y=10.0, z=5.0, radius=20.0)
        bad_lights = [dict(kind=2), dict(x=nan), dict(z=0.0), dict(relief=64.5), dict(ambient=-0.1), dict(diffuse=inf), dict(pt, x=32768.0),
                      dict(pt, radius=0.0), dict(pt, anchorDepth=255.5), dict(pt, anchorX=cols, anchorY=0)]
        for kw in bad_lights:                                                   # everything rtdd_simulate_relight refuses
            with pytest.raises(rt.RtddError) as e:
                c.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**kw), rt.Shadow())
            assert e.value.status == 1, kw
        bad_shadows = [dict(maxSteps=-1), dict(maxSteps=1025), dict(bias=-0.5), dict(bias=65537.0), dict(bias=nan), dict(bias=inf),
                       dict(softness=-1e-3), dict(softness=65537.0), dict(softness=nan), dict(softness=inf), dict(strength=-0.1),
                       dict(strength=1.5), dict(strength=nan), dict(strength=inf), dict(maxSteps=0, strength=2.0), dict(maxSteps=0, bias=nan)]
        for kw in bad_shadows:
            for L in (rt.Light(), rt.Light(**pt)):
                with pytest.raises(rt.RtddError) as e:
                    c.simulate_relight_shadowed(o, d, art, rows, cols, L, rt.Shadow(**kw))
                assert e.value.status == 1, kw
        for L, S in ((None, rt.Shadow()), (rt.Light(), None), (None, None)):    # null pointers
            with pytest.raises(rt.RtddError) as e:
                c.simulate_relight_shadowed(o, d, art, rows, cols, L, S)
            assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_relight_shadowed(o, d, o, rows, cols, rt.Light(), rt.Shadow())     # in place
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_relight_shadowed(o, d, art, 0, cols, rt.Light(), rt.Shadow(maxSteps=2000))   # the parameters are checked before the empty return
        assert e.value.status == 1
        c.simulate_relight_shadowed(o, d, o, 0, cols, rt.Light(), rt.Shadow())  # ... and the in-place rule after it
        assert_bad_images_refused(c, rt.lib().rtdd_simulate_relight_shadowed, o, d, art, rows, cols, (C.byref(rt.Light()), C.byref(rt.Shadow())))
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                             # nothing was launched
        for kw in (dict(maxSteps=1024, bias=65536.0, softness=65536.0, strength=1.0), dict(maxSteps=0, bias=0.0, softness=0.0, strength=0.0)):
            c.simulate_relight_shadowed(o, d, art, rows, cols, rt.Light(**pt), rt.Shadow(**kw))   # the bounds themselves are admitted
        c.synchronize()
        assert not np.array_equal(down(art), sentinel)


def test_harness_writes_the_restatements_image(tmp_path):
    bgr, ann = harness_pair(tmp_path, "png")
    with rt.Context(0) as c:                                                   # the harness's own depth map: the same estimate
        c.GPULoadWeights(0.4)
        estimate(c, bgr, ann)
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
    x, y = 300, 200
    point = light(POINT, x, y, 100, anchorX=x, anchorY=y, radius=200, relief=2, ambient=0.25, diffuse=1)
    directional = light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1)
    cases = [(["--shadows", "128"], directional, shadow(128)),
             (["--shadows", "300", "--shadow-bias", "0.5", "--shadow-softness", "0.75", "--shadow-strength", "0.875"], directional,
              shadow(300, 0.5, 0.75, 0.875)),
             (["--light-at", f"{x},{y}", "--shadows", "64", "--shadow-softness", "0.25"], point, shadow(64, softness=0.25)),
             (["--shadows", "0"], directional, shadow(0))]
    for args, L, S in cases:
        got = run_harness(tmp_path, "png", ["--effect", "relight"] + args)[1]
        assert_same_image(got, relight_shadowed(bgr, depth, L, S), args)
        assert np.array_equal(got, relight(bgr, depth, L)) == (S["maxSteps"] == 0)      # shadows are visible, and --shadows 0 is relight
    r = subprocess.run([harness_bin()] + harness_files(tmp_path, "png") + ["--effect", "relight", "--shadows", "2000"], capture_output=True, text=True)
    assert r.returncode != 0                                                   # refused by the library


def test_harness_refuses_live_with_shadows():
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3", "--effect", "relight", "--shadows", "64"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout


def test_harness_refuses_stray_shadow_options():
    for args, said in ((["--effect", "defocus", "--shadows", "64"], "--shadows needs --effect relight"),
                       (["--shadows", "64"], "--shadows needs --effect relight"),
                       (["--effect", "relight", "--shadow-softness", "0.5"], "need --shadows N")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout, (args, r.returncode, r.stdout)
