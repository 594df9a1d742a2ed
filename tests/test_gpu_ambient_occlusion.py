"""Ambient occlusion (include/rtdd.h rtdd_simulate_ambient_occlusion) on the GPU (-m gpu): byte for byte against the numpy restatement
of tests/ao_ref.py, which knows nothing of the kernel -- small and odd shapes and alignments, radii 1, 5 and 64 (larger than the image, a
halo over several tiles, an image smaller than a tile), both direction counts, both modes, no light, a directional and point lights; NaN
and out-of-range depths; the bounds of the parameters; the identities; the known answer of a wall; 1080p in full and bands of 4K and 8K;
padding bytes; sub-image views; FP contraction; the anchor pixel read on the device behind an estimate; the heal log; the host-side
refusals; the harness.  No tolerance anywhere: every operation of the header is a correctly rounded IEEE one."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import wild_depth
from ao_ref import MAP, SHADE, ambient, apply_ao, occluded, occlusion
from effect_gpu import ctx, dog_depth  # noqa: F401
from effect_gpu import (FILL, assert_bad_images_refused, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, harness_bin,
                        harness_files, harness_pair, padded_artistic, pixel_form_behind_estimate, random_inputs, run_harness, tile_mirrored)
from gpu_util import down, up
from relight_ref import DIRECTIONAL, POINT, light, relight, shade
from roi_util import FILL_INPUT, FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for

pytestmark = pytest.mark.gpu
F = np.float32


def _ao(A):
    return rt.AmbientOcclusion(**A)


def _run(c, o, d, rows, cols, A, L=None, align=512):
    art = up(np.full((rows, cols, 3), FILL, np.uint8), align)
    c.simulate_ambient_occlusion(o, d, art, rows, cols, _ao(A), rt.Light(**L) if L is not None else None)
    c.synchronize()
    return down(art)


def _relight(c, o, d, rows, cols, L):
    art = up(np.zeros((rows, cols, 3), np.uint8))
    c.simulate_relight(o, d, art, rows, cols, rt.Light(**L))
    c.synchronize()
    return down(art)


def _lights(rows, cols, relief):
    """A directional light; point lights inside and outside the image, anchored by value and by pixel."""
    common = dict(relief=relief, ambient=0.75, diffuse=1.5)
    ax, ay = cols // 3, rows - 1
    return [light(DIRECTIONAL, 3.5, -0.25, 0.5, color=(255, 128, 7), **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, cols + 40.0, 1.0, 25, anchorX=ax, anchorY=ay, radius=300, color=(10, 200, 255), **common)]


def _all_forms(c, o, d, orig, depth, rows, cols, A, align, what):
    """Every output of one occlusion: the shade, the map, and the three lights -- the restatement's ao computed once."""
    ao = ambient(depth, A)
    assert_same_image(_run(c, o, d, rows, cols, A, None, align), apply_ao(orig, ao, A), (what, A, "shade"))
    M = dict(A, mode=MAP)
    assert_same_image(_run(c, o, d, rows, cols, M, None, align), apply_ao(orig, ao, M), (what, M))
    for L in _lights(rows, cols, A["relief"]):
        assert_same_image(_run(c, o, d, rows, cols, A, L, align), apply_ao(orig, ao, A, L, shade(depth, L)), (what, A, L))
    return ao


# radius 64 exceeds most of these images; (130, 200) and (33, 70) have halos that cross several tiles both ways; (1, 1) .. (9, 1027) are
# smaller than one tile in a dimension; 255 / 257 / 1027 straddle the 64-pixel tile width
@pytest.mark.parametrize("shape,align", [((1, 1), 1), ((1, 37), 1), ((23, 1), 512), ((5, 255), 1), ((7, 257), 4), ((9, 1027), 1),
                                         ((130, 200), 512), ((33, 70), 4)])
def test_small_shapes_bit_exact(ctx, shape, align):
    rows, cols = shape
    orig, depth = random_inputs(rows, cols, rows * 1000 + cols)
    o, d = up(orig, align), up(depth, align)
    occluding = 0
    for radius in (1, 5, 64):
        for directions in (4, 8):
            A = occlusion(SHADE, directions, radius, 0.5, bias=0.25, strength=0.875)
            occluding += int((_all_forms(ctx, o, d, orig, depth, rows, cols, A, align, shape) < 1).any())
    assert occluding == (0 if rows * cols == 1 else 6)


def test_every_radius_class_and_its_neighbours(ctx):
    """The launcher chooses the LDS array by the radius: both sides of every threshold, on a smooth map whose creases are occluded."""
    rows, cols = 70, 150
    orig = random_inputs(rows, cols, 5)[0]
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    depth = (127.5 + 120 * np.sin(xx / 17.0) * np.cos(yy / 11.0)).astype(np.float32)
    o, d = up(orig, 1), up(depth, 1)
    L = _lights(rows, cols, 2.0)[0]
    shares = []
    for radius in (2, 8, 9, 16, 17, 32, 33, 63, 64):
        A = occlusion(SHADE, 8 if radius % 2 else 4, radius, 2.0, 0.125, 1.0)
        ao = ambient(depth, A)
        assert_same_image(_run(ctx, o, d, rows, cols, A, L, 1), apply_ao(orig, ao, A, L, shade(depth, L)), A)
        assert_same_image(_run(ctx, o, d, rows, cols, dict(A, mode=MAP), None, 1), apply_ao(orig, ao, dict(A, mode=MAP)), A)
        shares.append(float((ao < 1).mean()))
    assert 0.2 < min(shares) and max(shares) < 1.0


@pytest.mark.parametrize("name", ["out_of_range", "magnitudes", "huge", "infinite", "nan", "infinite_at_edges", "nan_at_edges"])
def test_out_of_range_and_non_finite_depths(ctx, name):
    rows, cols = 70, 133
    depth = wild_depth.make(name, rows, cols)["depth"]
    orig = random_inputs(rows, cols, 21)[0]
    o, d = up(orig), up(depth)
    for A in (occlusion(SHADE, 8, 5, 2.0, 0.0, 1.0), occlusion(SHADE, 4, 64, 0.25, 1.0, 0.5)):
        _all_forms(ctx, o, d, orig, depth, rows, cols, A, 512, name)


def test_extreme_parameters(ctx):
    """The bounds of the ranges: relief 64, bias 0 and 65536, strength 1, radius 64; a tiny relief whose rises are denormal."""
    rows, cols = 20, 140
    orig, depth = random_inputs(rows, cols, 23)
    o, d = up(orig), up(depth)
    for A in (occlusion(SHADE, 8, 64, 64.0, 0.0, 1.0), occlusion(SHADE, 8, 64, 64.0, 65536.0, 1.0), occlusion(SHADE, 4, 64, 64.0, 16000.0, 1.0),
              occlusion(SHADE, 8, 7, 1e-40, 0.0, 1.0), occlusion(SHADE, 4, 1, 64.0, 1e-30, 1.0)):
        ao = _all_forms(ctx, o, d, orig, depth, rows, cols, A, 512, "extreme")
        if A["bias"] == 65536.0:
            assert (ao == 1).all()
    assert (ambient(depth, occlusion(SHADE, 8, 64, 64.0, 0.0, 1.0)) < 0.05).any()        # a pit among walls: nearly black


def test_identities_on_the_device(ctx):
    rows, cols = 33, 300
    orig, depth = random_inputs(rows, cols, 22)
    const = np.full((rows, cols), 93.5, np.float32)
    o, d, dc = up(orig), up(depth), up(const)
    cases = [(d, occlusion(SHADE, 8, 0, 1.5, 0.0, 1.0)), (d, occlusion(SHADE, 4, 16, 1.5, 0.0, 0.0)), (d, occlusion(SHADE, 8, 64, 0.0, 0.0, 1.0)),
             (dc, occlusion(SHADE, 8, 16, 1.5, 0.0, 1.0)), (dc, occlusion(SHADE, 4, 64, 64.0, 0.0, 1.0))]
    for dev, A in cases:
        assert_same_image(_run(ctx, o, dev, rows, cols, A), orig, ("the original", A))
        assert (_run(ctx, o, dev, rows, cols, dict(A, mode=MAP)) == 255).all(), A
        for L in _lights(rows, cols, A["relief"]):
            want = _relight(ctx, o, dev, rows, cols, L)                 # rtdd_simulate_relight's own output, on the same context
            assert_same_image(_run(ctx, o, dev, rows, cols, A, L), want, ("relight", A, L))
    assert_same_image(_relight(ctx, o, d, rows, cols, _lights(rows, cols, 1.5)[0]), relight(orig, depth, _lights(rows, cols, 1.5)[0]), "relight")
    A = occlusion(SHADE, 8, 16, 1.5, 0.0, 1.0)                          # ... and a rough map under the same settings is occluded
    assert not np.array_equal(_run(ctx, o, d, rows, cols, A), orig)
    L = _lights(rows, cols, 1.5)[0]
    assert not np.array_equal(_run(ctx, o, d, rows, cols, A, L), _relight(ctx, o, d, rows, cols, L))


@pytest.mark.parametrize("radius", [1, 5, 64])
def test_known_answer_on_the_device(ctx, radius):
    """A wall nearer on the right (tests/test_ambient_occlusion_cpu.py): at its foot occ_0 = t / sqrtf(1 + t * t), on it ao == 1."""
    rows, cols, x0, a, b = 5, 200, 117, 200.0, 120.5
    depth = np.full((rows, cols), a, np.float32)
    depth[:, x0:] = b
    orig = np.full((rows, cols, 3), 200, np.uint8)
    o, d = up(orig), up(depth)
    for r, beta in ((1.0, 0.0), (2.5, 3.0), (64.0, 0.25)):
        t = F(F(F(r) * F(F(255) - F(b))) - F(F(r) * F(F(255) - F(a)))) - F(beta)
        occ0 = F(t / np.sqrt(F(F(1) + F(t * t))))
        ao = F(F(1) - F(F(1) * F(occ0 * F(0.25))))
        A = occlusion(SHADE, 4, radius, r, beta, 1.0)
        out = _run(ctx, o, d, rows, cols, A)
        assert (out[2, x0 - 1] == int(F(200) * ao)).all() and (out[:, x0:] == 200).all() and (out[:, :x0 - radius] == 200).all()
        m = _run(ctx, o, d, rows, cols, dict(A, mode=MAP))
        assert (m[2, x0 - 1] == int(F(255) * ao)).all() and (m[:, x0:] == 255).all()
        assert_same_image(out, occluded(orig, depth, A), A)


def _restate_rows(depth, A, y0, y1, workers=16):
    """ambient(rows=(y0, y1)) with the rows shared out over threads."""
    edges = np.linspace(y0, y1, min(workers, y1 - y0) + 1).astype(int)
    with ThreadPoolExecutor(workers) as ex:
        return np.concatenate(list(ex.map(lambda ab: ambient(depth, A, (int(ab[0]), int(ab[1]))), zip(edges[:-1], edges[1:]))), 0)


# every pixel at 1080p; at 4K and 8K a band of 512 rows, whose marches leave it and are restated on the rows they reach
@pytest.mark.parametrize("rows,cols,band", [(1080, 1920, (0, 1080)), (2160, 3840, (900, 1412)), (4320, 7680, (3000, 3512))])
def test_full_size(ctx, dog_depth, rows, cols, band):
    rng = np.random.default_rng(rows)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = tile_mirrored(dog_depth, rows, cols)
    o, d = up(orig), up(depth)
    L = light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.5, diffuse=1.0)
    y0, y1 = band
    s = shade(depth, L)[y0:y1]
    for radius in (16, 64):
        A = occlusion(SHADE, 8, radius, 2.0, 0.5, 1.0)
        pitch = cols * 3 + 512
        base, art = padded_artistic(rows, cols, pitch)
        ctx.simulate_ambient_occlusion(o, d, art, rows, cols, _ao(A), rt.Light(**L))
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        ao = _restate_rows(depth, A, y0, y1)
        share = float((ao < 1).mean())
        print(f"{rows} x {cols} rows {y0}-{y1} radius {radius}: {share:.3f} of the pixels occluded, mean ao {float(ao.mean()):.4f}")
        assert 0.0 < share < 1.0
        assert_same_image(down(art)[y0:y1], apply_ao(orig[y0:y1], ao, A, L, s), (rows, radius))


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 19, cols * 3 + 13
    orig, depth = random_inputs(rows, cols, 8)
    o, d = up(orig), up(depth)
    for A, L in ((occlusion(SHADE, 8, 5, 1.0, 0.0, 1.0), None), (occlusion(MAP, 4, 64, 1.0, 0.0, 1.0), None),
                 (occlusion(SHADE, 8, 20, 1.0, 0.5, 0.5), _lights(rows, cols, 1.0)[0]), (occlusion(SHADE, 4, 9, 1.0, 0.5, 0.5), _lights(rows, cols, 1.0)[2])):
        base, art = padded_artistic(rows, cols, pitch)
        ctx.simulate_ambient_occlusion(o, d, art, rows, cols, _ao(A), rt.Light(**L) if L else None)
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert_same_image(down(art), occluded(orig, depth, A, L), (A, L))


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
    L = _lights(rows, cols, 1.5)[2]
    forms = [(occlusion(SHADE, 8, 5, 1.5, 0.25, 1.0), None), (occlusion(MAP, 4, 64, 1.5, 0.0, 1.0), None), (occlusion(SHADE, 8, 12, 1.5, 0.25, 0.75), L)]
    wants = [occluded(orig, depth, A, Lf) for A, Lf in forms]
    combos = covering(7, 7, 7)
    assert len(combos) == 49
    for k, (io, idp, ia) in enumerate(combos):
        A, Lf = forms[k % 3]
        out = Roi(np.zeros_like(orig), *lay[2][ia], FILL_OUTPUT, seed=k, what=f"artistic (lead {lay[2][ia][0]}, pitch {lay[2][ia][1]})")
        ctx.simulate_ambient_occlusion(ins_o[io].img, ins_d[idp].img, out.img, rows, cols, _ao(A), rt.Light(**Lf) if Lf else None)
        ctx.synchronize()
        assert_same_image(out.result(), wants[k % 3], (shape, lay[0][io], lay[1][idp], lay[2][ia], A))
        ins_o[io].assert_unchanged(); ins_d[idp].assert_unchanged()


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 40, 500
    orig, depth = random_inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    for A, L in ((occlusion(SHADE, 8, 12, 3.0, 0.5, 1.0), None), (occlusion(MAP, 4, 40, 3.0, 0.0, 0.75), None),
                 (occlusion(SHADE, 8, 64, 3.0, 0.5, 1.0), _lights(rows, cols, 3.0)[0]), (occlusion(SHADE, 4, 7, 3.0, 0.5, 1.0), _lights(rows, cols, 3.0)[1])):
        try:
            outs = []
            for contract in (0, 1):
                ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                outs.append(_run(ctx, o, d, rows, cols, A, L))
        finally:
            ctx.set_option(rt.OPT_FP_CONTRACT, 1)
        assert np.array_equal(outs[0], outs[1])
        assert_same_image(outs[0], occluded(orig, depth, A, L), "contraction")


def test_anchor_pixel_is_read_behind_an_unsynchronised_estimate():
    A = occlusion(SHADE, 8, 24, 2.0, 0.5, 1.0)

    def over(x, y):
        return light(POINT, x, y, 60, anchorX=x, anchorY=y, radius=150, relief=2, ambient=0.6, diffuse=2.0)

    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        L = over(x, y) if value is None else dict(over(x, y), anchorX=-1, anchorY=-1, anchorDepth=value)
        c.simulate_ambient_occlusion(o, d, art, rows, cols, _ao(A), rt.Light(**L))

    bgr, depth, x, y, _, image = pixel_form_behind_estimate(call)
    assert_same_image(image, occluded(bgr, depth, A, over(x, y)), "pixel form")
    assert not np.array_equal(image, relight(bgr, depth, over(x, y)))


def test_ambient_occlusion_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = random_inputs(rows, cols, 2)[0]
    L1 = light(POINT, 100, 200, 40, anchorX=100, anchorY=200, radius=120, relief=2, ambient=0.6, diffuse=2.0, color=(255, 220, 180))
    A1, A2, A3 = occlusion(SHADE, 8, 20, 2.0, 0.5, 0.875), occlusion(SHADE, 4, 64, 3.0, 0.0, 1.0), occlusion(MAP, 8, 7, 1.0, 0.25, 1.0)

    def queue(c, o, d, arts):
        light1, ao1 = rt.Light(**L1), _ao(A1)
        c.simulate_ambient_occlusion(o, d, arts[0], rows, cols, ao1, light1)
        light1.kind, light1.relief, light1.x = 7, -1.0, float("nan")   # the call has read both: the record holds them by value
        ao1.radius, ao1.directions, ao1.bias, ao1.strength = -5, 3, float("nan"), 9.0
        c.simulate_ambient_occlusion(o, d, arts[1], rows, cols, _ao(A2), None)
        c.simulate_ambient_occlusion(o, d, arts[2], rows, cols, _ao(A3), None)

    solved, healed = clean_and_healed(queue, 3, orig)
    assert_same_image(healed[0], occluded(orig, solved, A1, L1), "healed, under a point light")
    assert_same_image(healed[1], occluded(orig, solved, A2), "healed, no light")
    assert_same_image(healed[2], occluded(orig, solved, A3), "healed, the map")
    assert not np.array_equal(healed[0], relight(orig, solved, L1)) and not np.array_equal(healed[1], orig)


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = random_inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    nan, inf = float("nan"), float("inf")
    AO, Li = rt.AmbientOcclusion, rt.Light
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)

        def refused(ao, li, rows=rows, src=o, dst=art):
            with pytest.raises(rt.RtddError) as e:
                c.simulate_ambient_occlusion(src, d, dst, rows, cols, ao, li)
            assert e.value.status == 1
        bad = [dict(mode=2), dict(mode=-1), dict(directions=0), dict(directions=6), dict(directions=16), dict(radius=-1), dict(radius=65),
               dict(relief=-0.5), dict(relief=64.5), dict(relief=nan), dict(relief=inf), dict(bias=-0.5), dict(bias=65537.0), dict(bias=nan),
               dict(bias=inf), dict(strength=-0.1), dict(strength=1.5), dict(strength=nan), dict(strength=-inf), dict(radius=0, strength=2.0),
               dict(radius=0, bias=nan)]
        for kw in bad:
            refused(AO(**kw), None)
            refused(AO(**kw), Li(relief=kw.get("relief", 1.0)))
        refused(None, None); refused(None, Li())                                # a null ao
        refused(AO(mode=rt.AO_MAP), Li())                                       # the map takes no light
        pt = dict(kind=POINT, x=10.0, y=10.0, z=5.0, radius=20.0)
        bad_lights = [dict(kind=2), dict(x=nan), dict(z=0.0), dict(relief=64.5), dict(ambient=-0.1), dict(diffuse=inf), dict(pt, x=32768.0),
                      dict(pt, radius=0.0), dict(pt, anchorDepth=255.5), dict(pt, anchorX=cols, anchorY=0)]
        for kw in bad_lights:                                                   # everything rtdd_simulate_relight refuses
            refused(AO(relief=kw.get("relief", 1.0)), Li(**kw))
        refused(AO(relief=1.0), Li(relief=1.5))                                 # the two reliefs differ
        refused(AO(relief=1.0), Li(relief=float(np.nextafter(F(1), F(2)))))
        refused(AO(relief=0.0), Li(relief=-0.0))                                # ... bit for bit
        refused(AO(), None, src=o, dst=o); refused(AO(), Li(), src=o, dst=o)    # in place
        refused(AO(mode=rt.AO_MAP), None, src=o, dst=o)
        refused(AO(radius=100), None, rows=0)                                   # the parameters are checked before the empty return
        c.simulate_ambient_occlusion(o, d, o, 0, cols, AO(), None)              # ... and the in-place rule after it
        f = rt.lib().rtdd_simulate_ambient_occlusion
        for ao, li in ((C.byref(AO()), None), (C.byref(AO()), C.byref(Li())), (C.byref(AO(mode=rt.AO_MAP)), None)):
            assert_bad_images_refused(c, f, o, d, art, rows, cols, (ao, li))    # (the map does not read `original`, and still wants one)
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                             # nothing was launched
        for kw in (dict(radius=64, relief=64.0, bias=65536.0, strength=1.0), dict(radius=0, relief=0.0, bias=0.0, strength=0.0, directions=4)):
            c.simulate_ambient_occlusion(o, d, art, rows, cols, AO(**kw), Li(relief=kw["relief"], **pt))      # the bounds themselves are admitted
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
    cases = [(["--effect", "ao"], occlusion(SHADE, 8, 16, 2.0, 0.0, 1.0), None),
             (["--effect", "ao", "--ao-radius", "40", "--ao-directions", "4", "--ao-bias", "0.5", "--ao-strength", "0.75", "--relief", "3"],
              occlusion(SHADE, 4, 40, 3.0, 0.5, 0.75), None),
             (["--effect", "ao", "--ao-map", "--ao-radius", "8"], occlusion(MAP, 8, 8, 2.0, 0.0, 1.0), None),
             (["--effect", "relight", "--ao", "24"], occlusion(SHADE, 8, 24, 2.0, 0.0, 1.0), directional),
             (["--effect", "relight", "--light-at", f"{x},{y}", "--ao", "12", "--ao-directions", "4", "--ao-bias", "1", "--ao-strength", "0.5"],
              occlusion(SHADE, 4, 12, 2.0, 1.0, 0.5), point),
             (["--effect", "relight", "--ao", "0"], occlusion(SHADE, 8, 0, 2.0, 0.0, 1.0), directional)]
    for args, A, L in cases:
        got = run_harness(tmp_path, "png", args)[1]
        assert_same_image(got, occluded(bgr, depth, A, L), args)
        plain = relight(bgr, depth, L) if L is not None else bgr
        assert np.array_equal(got, plain) == (A["radius"] == 0)                 # the occlusion is visible, and --ao 0 is relight
    r = subprocess.run([harness_bin()] + harness_files(tmp_path, "png") + ["--effect", "ao", "--ao-radius", "65"], capture_output=True, text=True)
    assert r.returncode != 0                                                   # refused by the library


def test_harness_refuses_the_misuses():
    for args, said in ((["--effect", "relight", "--ao", "16", "--shadows", "64"], "--ao and --shadows cannot be combined"),
                       (["--effect", "relight", "--ao-bias", "0.5"], "need --ao R or --effect ao"),
                       (["--effect", "defocus", "--ao-strength", "0.5"], "need --ao R or --effect ao"),
                       (["--ao-directions", "4"], "need --ao R or --effect ao"),
                       (["--effect", "relight", "--ao-radius", "8"], "need --effect ao"),
                       (["--effect", "haze", "--ao-map"], "need --effect ao"),
                       (["--effect", "ao", "--ao", "16"], "--ao needs --effect relight"),
                       (["--ao", "16"], "--ao needs --effect relight")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and said in r.stdout, (args, r.returncode, r.stdout)
    for args in (["--effect", "ao"], ["--effect", "relight", "--ao", "16"]):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "not supported with --live" in r.stdout, (args, r.stdout)
