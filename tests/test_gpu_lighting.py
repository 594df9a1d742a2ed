"""The whole lighting model in one call (include/rtdd.h rtdd_simulate_lighting) on the GPU (-m gpu): byte for byte against the numpy
restatement of tests/lighting_ref.py, which composes the restatements of the calls it fuses and knows nothing of the kernel -- small and
odd shapes round the 64 x 16 tile and alignments, both light kinds, hard and soft shadows, 4 and 8 directions; every radius class and
its neighbours crossed with marches shorter than, as long as and longer than the staged halo; point lights inside, far outside, below
the surface and anchored at a pixel; NaN, infinite and out-of-range depths; the bounds of the parameters; the three identities against
the three existing entry points' own output; FP contraction; padding bytes and sub-image views; the anchor pixel read on the device
behind an estimate; the heal log; the host-side refusals; a band of 1080p and of 4K; the harness.  No tolerance anywhere: every
operation of the header is a correctly rounded IEEE one."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import wild_depth
from ao_ref import SHADE, occluded, occlusion
from effect_gpu import ctx, dog_depth  # noqa: F401
from effect_gpu import (FILL, assert_bad_images_refused, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, harness_bin,
                        harness_files, harness_pair, padded_artistic, pixel_form_behind_estimate, random_inputs, run_harness, tile_mirrored)
from gpu_util import down, up
from lighting_ref import lighting
from relight_ref import DIRECTIONAL, POINT, light, relight
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from shadow_ref import relight_shadowed, shadow

pytestmark = pytest.mark.gpu
F = np.float32


def _call(c, o, d, art, rows, cols, L, S, A):
    c.simulate_lighting(o, d, art, rows, cols, rt.Light(**L), rt.Shadow(**S), rt.AmbientOcclusion(**A))


def _run(c, o, d, rows, cols, L, S, A, align=512):
    art = up(np.full((rows, cols, 3), FILL, np.uint8), align)
    _call(c, o, d, art, rows, cols, L, S, A)
    c.synchronize()
    return down(art)


def _lights(rows, cols, relief):
    """A diagonal directional light and one along a major axis; point lights inside and outside the image, anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.75, diffuse=1.5)
    ax, ay = cols // 3, rows - 1
    return [light(DIRECTIONAL, -1, -1, 1, color=(255, 128, 7), **common),
            light(DIRECTIONAL, 3.5, -0.25, 0.5, **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, cols + 40.0, 1.0, 25, anchorX=ax, anchorY=ay, radius=300, color=(10, 200, 255), **common)]


def _smooth(rows, cols):
    """A smooth map whose ridges throw long shadows and whose creases are occluded."""
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    return (127.5 + 120 * np.sin(xx / 17.0) * np.cos(yy / 11.0)).astype(np.float32)


# the tile is 64 x 16: 255 / 257 / 1027 / 65 / 129 straddle its width, 17 and 33 its height; (1, 1) .. (9, 1027) are smaller than one
# tile in a dimension; radius 64 exceeds most of these images
@pytest.mark.parametrize("shape,align", [((1, 1), 1), ((1, 37), 1), ((23, 1), 512), ((5, 255), 1), ((7, 257), 4), ((9, 1027), 1),
                                         ((17, 65), 512), ((33, 129), 4)])
def test_small_shapes_bit_exact(ctx, shape, align):
    rows, cols = shape
    orig, depth = random_inputs(rows, cols, rows * 1000 + cols)
    o, d = up(orig, align), up(depth, align)
    n = 0
    for L in _lights(rows, cols, 0.5):
        for softness in (0.0, 0.75):
            for directions in (4, 8):
                S = shadow(64, bias=0.25, softness=softness, strength=0.875)
                A = occlusion(SHADE, directions, (1, 5, 20, 64)[n % 4], 0.5, bias=0.25, strength=0.875)
                n += 1
                assert_same_image(_run(ctx, o, d, rows, cols, L, S, A, align), lighting(orig, depth, L, S, A), (shape, L, S, A))


@pytest.mark.parametrize("radius", [1, 8, 9, 16, 17, 32, 33, 64])
def test_every_radius_class_and_its_neighbours(ctx, radius):
    """The launcher chooses the LDS array by the radius; the march is as long as the staged halo, one shorter, one longer, a single
    step, and 1024 steps: on 40 x 200 rays start inside a tile, cross the halo into the map beyond it, and leave the image."""
    rows, cols = 40, 200
    orig = random_inputs(rows, cols, 5)[0]
    depth = _smooth(rows, cols)
    o, d = up(orig, 1), up(depth, 1)
    common = dict(relief=2.0, ambient=0.75, diffuse=1.5)
    lights = [light(DIRECTIONAL, 3.5, -0.25, 0.5, **common), light(POINT, cols + 40.0, 1.0, 25, anchorX=70, anchorY=39, radius=300, **common)]
    for steps in sorted({1, max(radius - 1, 1), radius, radius + 1, 1024}):
        for i, L in enumerate(lights):
            S = shadow(steps, bias=0.125, softness=4.0 * ((i + steps) % 2), strength=1.0)
            A = occlusion(SHADE, 8 if radius % 2 else 4, radius, 2.0, 0.125, 1.0)
            want = lighting(orig, depth, L, S, A)
            assert_same_image(_run(ctx, o, d, rows, cols, L, S, A, 1), want, (L, S, A))
            assert not np.array_equal(want, occluded(orig, depth, A, L)) and not np.array_equal(want, relight_shadowed(orig, depth, L, S))


def test_point_lights(ctx):
    """Inside the image (the march ends at the light's column or row), far outside, below the surface, anchored at a pixel."""
    rows, cols = 33, 129
    orig, depth = random_inputs(rows, cols, 41)
    smooth = _smooth(rows, cols)
    common = dict(relief=1.5, ambient=0.5, diffuse=2.0)
    lights = [light(POINT, 70.25, 12.5, 10, anchorDepth=100, radius=40, **common),
              light(POINT, 3.0, 30.0, 40, anchorDepth=30, radius=80, **common),
              light(POINT, -3000.5, rows + 7.25, 2000, anchorDepth=255, radius=5000, color=(10, 200, 255), **common),
              light(POINT, 30000.0, -20000.0, 60000, anchorDepth=0, radius=65536, **common),
              light(POINT, 40.5, 2.5, 1e-3, anchorDepth=255, radius=60, **common),                       # below the surface
              light(POINT, 100.0, 20.0, 0.5, anchorX=100, anchorY=20, radius=30, **common),              # at the height of its anchor pixel
              light(POINT, cols + 40.0, 1.0, 25, anchorX=0, anchorY=0, radius=300, **common)]
    for dmap in (depth, smooth):
        o, d = up(orig), up(dmap)
        for i, L in enumerate(lights):
            S = shadow(1024, bias=0.125, softness=0.5 * (i % 2), strength=0.875)
            A = occlusion(SHADE, 8, (12, 33)[i % 2], 1.5, 0.25, 1.0)
            assert_same_image(_run(ctx, o, d, rows, cols, L, S, A), lighting(orig, dmap, L, S, A), (L, S, A))


@pytest.mark.parametrize("name", ["out_of_range", "magnitudes", "huge", "infinite", "nan", "infinite_at_edges", "nan_at_edges"])
def test_out_of_range_and_non_finite_depths(ctx, name):
    rows, cols = 70, 133
    depth = wild_depth.make(name, rows, cols)["depth"]
    orig = random_inputs(rows, cols, 21)[0]
    o, d = up(orig), up(depth)
    for L, S, A in ((_lights(rows, cols, 2.0)[0], shadow(200, softness=0.5), occlusion(SHADE, 8, 5, 2.0, 0.0, 1.0)),
                    (_lights(rows, cols, 0.25)[3], shadow(1024, bias=0.5), occlusion(SHADE, 4, 64, 0.25, 1.0, 0.5))):
        assert_same_image(_run(ctx, o, d, rows, cols, L, S, A), lighting(orig, depth, L, S, A), (name, L, S, A))


def test_extreme_parameters(ctx):
    """The bounds of the ranges: relief 64, bias 65536 (of either march), softness 65536, strength 0 and 1, 1024 steps, radius 64."""
    rows, cols = 20, 140
    orig, depth = random_inputs(rows, cols, 23)
    o, d = up(orig), up(depth)
    Ld = light(DIRECTIONAL, -1, 0.5, 0.05, relief=64, ambient=0.75, diffuse=1.5)
    Lp = light(POINT, 32767, -32768, 65536, anchorDepth=0, radius=65536, relief=64, ambient=8.0, diffuse=8.0)
    Ln = light(POINT, 70.0, 6.0, 1e-30, anchorDepth=255, radius=10, relief=64, ambient=0.75, diffuse=1.5)
    cases = [(Ld, shadow(1024, 0.0, 0.0, 1.0), occlusion(SHADE, 8, 64, 64.0, 0.0, 1.0)),
             (Ld, shadow(1024, 65536.0, 0.0, 1.0), occlusion(SHADE, 8, 64, 64.0, 0.5, 1.0)),
             (Ld, shadow(1024, 0.0, 65536.0, 1.0), occlusion(SHADE, 4, 64, 64.0, 65536.0, 1.0)),
             (Ld, shadow(1024, 0.0, 1e-40, 1.0), occlusion(SHADE, 8, 1, 64.0, 1e-30, 1.0)),
             (Lp, shadow(1024, 0.0, 0.5, 1.0), occlusion(SHADE, 8, 64, 64.0, 0.0, 1.0)),
             (Ln, shadow(1024, 1e-30, 0.0, 1.0), occlusion(SHADE, 4, 33, 64.0, 16000.0, 1.0)),
             (Ld, shadow(1024, 0.0, 0.0, 0.0), occlusion(SHADE, 8, 64, 64.0, 0.0, 1.0)),             # strength 0 of either term
             (Ld, shadow(1024, 0.0, 0.0, 1.0), occlusion(SHADE, 8, 64, 64.0, 0.0, 0.0))]
    for L, S, A in cases:
        assert_same_image(_run(ctx, o, d, rows, cols, L, S, A), lighting(orig, depth, L, S, A), (L, S, A))


def test_identities_on_the_device(ctx):
    """Against the three existing entry points' own output, on the same context."""
    rows, cols = 33, 300
    orig, depth = random_inputs(rows, cols, 22)
    o, d = up(orig), up(depth)
    S, A = shadow(64, bias=0.125, softness=0.5, strength=0.75), occlusion(SHADE, 8, 16, 1.5, 0.25, 0.875)

    def other(f, *tail):
        art = up(np.zeros((rows, cols, 3), np.uint8))
        f(o, d, art, rows, cols, *tail)
        ctx.synchronize()
        return down(art)

    lights = _lights(rows, cols, 1.5)
    for L in lights:
        Lc = rt.Light(**L)
        plain = other(ctx.simulate_relight, Lc)
        shadowed = other(ctx.simulate_relight_shadowed, Lc, rt.Shadow(**S))
        under = other(ctx.simulate_ambient_occlusion, rt.AmbientOcclusion(**A), Lc)
        for S0 in (dict(S, maxSteps=0), dict(S, strength=0.0)):
            assert_same_image(_run(ctx, o, d, rows, cols, L, S0, A), under, ("ambient occlusion under the light", L, S0))
        for A0 in (dict(A, radius=0), dict(A, strength=0.0)):
            assert_same_image(_run(ctx, o, d, rows, cols, L, S, A0), shadowed, ("relight_shadowed", L, A0))
            for S0 in (dict(S, maxSteps=0), dict(S, strength=0.0)):
                assert_same_image(_run(ctx, o, d, rows, cols, L, S0, A0), plain, ("relight", L, S0, A0))
        if L is lights[0] or L is lights[2]:                             # the kernel itself, not the launcher's shortcuts: k_lighting runs ...
            # ... with a bias no horizon can clear (ao == 1 exactly), and with one no step can occlude under (q == 0)
            assert_same_image(_run(ctx, o, d, rows, cols, L, S, dict(A, bias=65536.0)), shadowed, ("k_lighting, ao == 1", L))
            assert_same_image(_run(ctx, o, d, rows, cols, L, dict(S, bias=65536.0), A), under, ("k_lighting, q == 0", L))
        full = _run(ctx, o, d, rows, cols, L, S, A)                      # ... and with both terms it is none of the three
        assert not np.array_equal(full, under) and not np.array_equal(full, shadowed) and not np.array_equal(full, plain)
    up_ = light(DIRECTIONAL, 0, 0, 3, relief=1.5, ambient=0.75, diffuse=1.5)    # the light straight above (m == 0) casts no shadow
    assert_same_image(_run(ctx, o, d, rows, cols, up_, S, A), occluded(orig, depth, A, up_), "m == 0")
    flat = light(DIRECTIONAL, -1, -1, 1, relief=0.0, ambient=0.75, diffuse=1.5)  # a flat surface: neither term
    assert_same_image(_run(ctx, o, d, rows, cols, flat, S, dict(A, relief=0.0)), relight(orig, depth, flat), "relief 0")


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 40, 500
    orig, depth = random_inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    lights = _lights(rows, cols, 3.0)
    for L, S, A in ((lights[0], shadow(100, 0.5, 0.5, 1.0), occlusion(SHADE, 8, 12, 3.0, 0.5, 1.0)),
                    (lights[2], shadow(100, 0.0, 0.0, 0.75), occlusion(SHADE, 4, 40, 3.0, 0.0, 0.75))):
        try:
            outs = []
            for contract in (0, 1):
                ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                outs.append(_run(ctx, o, d, rows, cols, L, S, A))
        finally:
            ctx.set_option(rt.OPT_FP_CONTRACT, 1)
        assert np.array_equal(outs[0], outs[1])
        assert_same_image(outs[0], lighting(orig, depth, L, S, A), "contraction")


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 19, cols * 3 + 13
    orig, depth = random_inputs(rows, cols, 8)
    o, d = up(orig), up(depth)
    lights = _lights(rows, cols, 1.0)
    for L, S, A in ((lights[0], shadow(64), occlusion(SHADE, 8, 5, 1.0, 0.0, 1.0)), (lights[3], shadow(300, 0.5, 0.5, 0.5), occlusion(SHADE, 4, 64, 1.0, 0.5, 0.5)),
                    (lights[1], shadow(64), occlusion(SHADE, 8, 0, 1.0, 0.0, 1.0)), (lights[2], shadow(0), occlusion(SHADE, 8, 20, 1.0, 0.0, 1.0))):
        base, art = padded_artistic(rows, cols, pitch)
        _call(ctx, o, d, art, rows, cols, L, S, A)
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert_same_image(down(art), lighting(orig, depth, L, S, A), (L, S, A))


@pytest.mark.parametrize("shape", [(9, 67), (13, 131), (1, 7), (7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sub_image_views(ctx, shape):
    """Input and output are views into larger allocations (tests/roi_util.py), every layout of each image and every pair of layouts of
    any two: the pixels are the restatement's, every byte around the output still holds its fill, and the inputs' parents are unchanged."""
    rows, cols = shape
    orig, depth = random_inputs(rows, cols, 31 + rows)
    lay = [[(lead, pitch_for(cols * 3, lead, res)) for lead, res in LAYOUTS_U8], [(lead, pitch_for(cols * 4, lead, res)) for lead, res in LAYOUTS_F32],
           [(lead, pitch_for(cols * 3, lead, res)) for lead, res in LAYOUTS_U8]]
    ins_o = [Roi(orig, lead, pitch, FILL_INPUT, what=f"original (lead {lead}, pitch {pitch})") for lead, pitch in lay[0]]
    ins_d = [Roi(depth, lead, pitch, FILL_INPUT, what=f"depth (lead {lead}, pitch {pitch})") for lead, pitch in lay[1]]
    lights = _lights(rows, cols, 1.5)
    forms = [(lights[0], shadow(64, 0.25, 0.5, 1.0), occlusion(SHADE, 8, 5, 1.5, 0.25, 1.0)),
             (lights[3], shadow(200, 0.0, 0.0, 0.75), occlusion(SHADE, 4, 64, 1.5, 0.0, 1.0)),
             (lights[2], shadow(64, 0.25, 0.5, 1.0), occlusion(SHADE, 8, 12, 1.5, 0.25, 0.75))]
    wants = [lighting(orig, depth, L, S, A) for L, S, A in forms]
    combos = covering(7, 7, 7)
    assert len(combos) == 49
    for k, (io, idp, ia) in enumerate(combos):
        L, S, A = forms[k % 3]
        out = Roi(np.zeros_like(orig), *lay[2][ia], FILL_OUTPUT, seed=k, what=f"artistic (lead {lay[2][ia][0]}, pitch {lay[2][ia][1]})")
        _call(ctx, ins_o[io].img, ins_d[idp].img, out.img, rows, cols, L, S, A)
        ctx.synchronize()
        assert_same_image(out.result(), wants[k % 3], (shape, lay[0][io], lay[1][idp], lay[2][ia], A))
        ins_o[io].assert_unchanged(); ins_d[idp].assert_unchanged()


def test_anchor_pixel_is_read_behind_an_unsynchronised_estimate():
    S, A = shadow(96, bias=0.5, softness=0.5, strength=0.875), occlusion(SHADE, 8, 24, 2.0, 0.5, 1.0)

    def over(x, y):
        return light(POINT, x, y, 60, anchorX=x, anchorY=y, radius=150, relief=2, ambient=0.6, diffuse=2.0)

    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        L = over(x, y) if value is None else dict(over(x, y), anchorX=-1, anchorY=-1, anchorDepth=value)
        _call(c, o, d, art, rows, cols, L, S, A)

    bgr, depth, x, y, _, image = pixel_form_behind_estimate(call)
    assert_same_image(image, lighting(bgr, depth, over(x, y), S, A), "pixel form")
    assert not np.array_equal(image, occluded(bgr, depth, A, over(x, y))) and not np.array_equal(image, relight_shadowed(bgr, depth, over(x, y), S))


def test_lighting_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = random_inputs(rows, cols, 2)[0]
    L1 = light(POINT, 100, 200, 40, anchorX=100, anchorY=200, radius=120, relief=2, ambient=0.6, diffuse=2.0, color=(255, 220, 180))
    L2 = light(DIRECTIONAL, 1, -2, 1.5, relief=3, ambient=0.5, diffuse=1.25)
    S1, S2 = shadow(96, bias=0.5, softness=0.5, strength=0.875), shadow(200)
    A1, A2 = occlusion(SHADE, 8, 20, 2.0, 0.5, 0.875), occlusion(SHADE, 4, 64, 3.0, 0.0, 1.0)

    def queue(c, o, d, arts):
        light1, shadow1, ao1 = rt.Light(**L1), rt.Shadow(**S1), rt.AmbientOcclusion(**A1)
        c.simulate_lighting(o, d, arts[0], rows, cols, light1, shadow1, ao1)
        light1.kind, light1.relief, light1.x = 7, -1.0, float("nan")   # the call has read all three: the record holds them by value
        shadow1.maxSteps, shadow1.softness = -3, float("nan")
        ao1.radius, ao1.directions, ao1.bias, ao1.strength = -5, 3, float("nan"), 9.0
        _call(c, o, d, arts[1], rows, cols, L2, S2, A2)

    solved, healed = clean_and_healed(queue, 2, orig)
    assert_same_image(healed[0], lighting(orig, solved, L1, S1, A1), "healed, under a point light")
    assert_same_image(healed[1], lighting(orig, solved, L2, S2, A2), "healed, under a directional light")
    assert not np.array_equal(healed[0], occluded(orig, solved, A1, L1)) and not np.array_equal(healed[1], relight_shadowed(orig, solved, L2, S2))


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = random_inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    nan, inf = float("nan"), float("inf")
    AO, Li, Sh = rt.AmbientOcclusion, rt.Light, rt.Shadow
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)

        def refused(li, sh, ao, rows=rows, src=o, dst=art):
            with pytest.raises(rt.RtddError) as e:
                c.simulate_lighting(src, d, dst, rows, cols, li, sh, ao)
            assert e.value.status == 1
        refused(None, Sh(), AO()); refused(Li(), None, AO()); refused(Li(), Sh(), None)      # each of the three pointers null
        refused(Li(), Sh(), AO(mode=rt.AO_MAP))                                              # the map is not a lighting term
        refused(Li(), Sh(), AO(mode=2)); refused(Li(), Sh(), AO(mode=-1))
        refused(Li(relief=1.5), Sh(), AO(relief=1.0))                                        # the two reliefs differ
        refused(Li(relief=float(np.nextafter(F(1), F(2)))), Sh(), AO(relief=1.0))
        refused(Li(relief=-0.0), Sh(), AO(relief=0.0))                                       # ... bit for bit
        pt = dict(kind=POINT, x=10.0, y=10.0, z=5.0, radius=20.0)
        bad_lights = [dict(kind=2), dict(x=nan), dict(z=0.0), dict(relief=64.5), dict(ambient=-0.1), dict(diffuse=inf), dict(pt, x=32768.0),
                      dict(pt, radius=0.0), dict(pt, anchorDepth=255.5), dict(pt, anchorX=cols, anchorY=0)]
        for kw in bad_lights:                                                   # everything rtdd_simulate_relight refuses
            refused(Li(**kw), Sh(), AO(relief=kw.get("relief", 1.0)))
        bad_shadows = [dict(maxSteps=-1), dict(maxSteps=1025), dict(bias=-0.5), dict(bias=65537.0), dict(bias=nan), dict(softness=-1.0),
                       dict(softness=inf), dict(strength=-0.1), dict(strength=1.5), dict(strength=nan), dict(maxSteps=0, strength=2.0)]
        for kw in bad_shadows:                                                  # everything rtdd_simulate_relight_shadowed refuses
            refused(Li(), Sh(**kw), AO())
        bad_aos = [dict(directions=0), dict(directions=6), dict(directions=16), dict(radius=-1), dict(radius=65), dict(relief=nan), dict(bias=-0.5),
                   dict(bias=65537.0), dict(bias=nan), dict(bias=inf), dict(strength=-0.1), dict(strength=1.5), dict(strength=nan),
                   dict(radius=0, strength=2.0), dict(radius=0, bias=nan)]
        for kw in bad_aos:                                                      # everything rtdd_simulate_ambient_occlusion refuses under a light
            refused(Li(), Sh(), AO(**kw))
        refused(Li(), Sh(), AO(), src=o, dst=o)                                 # in place
        refused(Li(), Sh(maxSteps=2000), AO(), rows=0)                          # the parameters are checked before the empty return
        c.simulate_lighting(o, d, o, 0, cols, Li(), Sh(), AO())                 # ... and the in-place rule after it
        f = rt.lib().rtdd_simulate_lighting
        assert_bad_images_refused(c, f, o, d, art, rows, cols, (C.byref(Li()), C.byref(Sh()), C.byref(AO())))
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                             # nothing was launched
        c.simulate_lighting(o, d, art, rows, cols, Li(relief=64.0, **pt), Sh(1024, 65536.0, 65536.0, 1.0),
                            AO(radius=64, relief=64.0, bias=65536.0, strength=1.0))                            # the bounds themselves are admitted
        c.synchronize()
        assert not np.array_equal(down(art), sentinel)


# one band of 128 rows at size, whose marches leave it and are restated on the rows they reach
@pytest.mark.parametrize("rows,cols,band", [(1080, 1920, (500, 628)), (2160, 3840, (900, 1028))])
def test_a_band_at_size(ctx, dog_depth, rows, cols, band):
    rng = np.random.default_rng(rows)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = tile_mirrored(dog_depth, rows, cols)
    o, d = up(orig), up(depth)
    L = light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.5, diffuse=1.0)
    S, A = shadow(64, bias=0.5), occlusion(SHADE, 8, 16, 2.0, 0.5, 1.0)
    base, art = padded_artistic(rows, cols, cols * 3 + 512)
    _call(ctx, o, d, art, rows, cols, L, S, A)
    ctx.synchronize()
    assert_padding_untouched(base, cols)
    y0, y1 = band
    want = lighting(orig, depth, L, S, A, rows=band)
    assert_same_image(down(art)[y0:y1], want, (rows, band))
    assert not np.array_equal(want, occluded(orig, depth, A, L, rows=band)) and not np.array_equal(want, relight_shadowed(orig, depth, L, S, rows=band))


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
    cases = [(["--effect", "lighting"], directional, shadow(256), occlusion(SHADE, 8, 16, 2.0, 0.0, 1.0)),
             (["--effect", "lighting", "--light-at", f"{x},{y}", "--shadows", "128", "--shadow-bias", "0.5", "--shadow-softness", "0.75", "--shadow-strength",
               "0.875", "--ao", "12", "--ao-directions", "4", "--ao-bias", "1", "--ao-strength", "0.5"], point, shadow(128, 0.5, 0.75, 0.875),
              occlusion(SHADE, 4, 12, 2.0, 1.0, 0.5))]
    for args, L, S, A in cases:
        got = run_harness(tmp_path, "png", args)[1]
        assert_same_image(got, lighting(bgr, depth, L, S, A), args)
        assert not np.array_equal(got, occluded(bgr, depth, A, L)) and not np.array_equal(got, relight_shadowed(bgr, depth, L, S))


def test_harness_refuses_the_misuses():
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--effect", "relight", "--ao", "16", "--shadows", "64"], capture_output=True, text=True)
    assert r.returncode == 1 and "--ao and --shadows cannot be combined" in r.stdout and "--effect lighting" in r.stdout, r.stdout
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3", "--effect", "lighting"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout, r.stdout
    for args, said in ((["--effect", "lighting", "--ao-radius", "8"], "need --effect ao"), (["--effect", "lighting", "--ao-map"], "need --effect ao")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout, (args, r.stdout)
