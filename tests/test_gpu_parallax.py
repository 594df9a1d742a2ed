"""The 2-D parallax view (include/rtdd.h rtdd_simulate_parallax) on the GPU (-m gpu): bit for bit against the numpy restatement of
tests/parallax_ref.py, which knows nothing of the kernels' waves and launches -- small and odd shapes, one that crosses workgroups in
both directions, rows wider than 1024 and whole rows of holes; adversarial maps; shifts and dolly at their bounds; ties; the stereo
identity on the device; determinism and FP contraction; sub-image views; the shared scratch buffer; the zero-parallax pixel read on the
device behind an estimate; the heal log; the host-side refusals; the harness."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from effect_gpu import ctx  # noqa: F401
from effect_gpu import (assert_bad_images_refused, assert_padding_untouched, assert_same_image, clean_and_healed, estimate, harness_bin,
                        harness_pair, padded_artistic, pixel_form_behind_estimate, raw_images, run_harness)
from gpu_util import down, up
from parallax_ref import parallax, scatter
from roi_util import FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from stereo_ref import stereo

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 64), (5, 97), (61, 83), (257, 300), (4, 2100), (3, 500)]
Z0 = [0.0, 127.5, 255.0]


def _orig(rows, cols, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def _maps(rows, cols, seed):
    """random in [-20, 280] with NaN and +-inf entries; a near disc on a far ground; a ramp; constant maps."""
    rng = np.random.default_rng(seed)
    rnd = rng.uniform(-20, 280, (rows, cols)).astype(np.float32)
    u = rng.random((rows, cols))
    rnd[u < 0.03] = np.nan
    rnd[(u > 0.03) & (u < 0.04)] = np.inf
    rnd[(u > 0.04) & (u < 0.05)] = -np.inf
    yy, xx = np.mgrid[0:rows, 0:cols]
    r = max(min(rows, cols) / 3.0, 1.0)
    disc = np.where((xx - cols / 2.0) ** 2 + (yy - rows / 2.0) ** 2 <= r * r, 10.0, 240.0).astype(np.float32)
    ramp = ((xx + 2 * yy) * (255.0 / max(cols + 2 * rows - 3, 1))).astype(np.float32)
    return {"random": rnd, "disc": disc, "ramp": ramp, "near": np.zeros((rows, cols), np.float32), "far": np.full((rows, cols), 255.0, np.float32)}


def _dolly_bound(rows, cols):
    """The largest f32 dolly the header admits: |dolly| * max(cols - 1, rows - 1) / 2 <= 256 in double."""
    span = max(cols - 1, rows - 1)
    if span == 0:
        return 1.0
    d = np.float32(512.0 / span)
    if float(d) * span / 2.0 > 256.0:
        d = np.nextafter(d, np.float32(0))
    return float(d)


def _views(rows, cols):
    """(shiftX, shiftY, dolly): shifts at +-256 and at small odd values, on both axes and mixed; dolly at both signs, up to the bound."""
    b = _dolly_bound(rows, cols)
    return [(256, 0, 0.0), (0, -256, 0.0), (-256, 256, 0.0), (7, 0, 0.0), (0, 5, 0.0), (-3, 9, 0.0), (19, -37, 0.0),
            (0, 0, b), (0, 0, -b), (0, 0, float(np.float32(b * 0.37))), (256, -256, b), (-5, 3, -b), (256, 0, float(np.float32(b * 0.5)))]


def _run(c, o, d, rows, cols, view, z0=0.0, at=None, align=512):
    art = up(np.zeros((rows, cols, 3), np.uint8), align)
    x, y = at if at is not None else (-1, -1)
    c.simulate_parallax(o, d, art, rows, cols, rt.Parallax(view[0], view[1], view[2], z0, x, y))
    c.synchronize()
    return down(art)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_exact(ctx, shape):
    rows, cols = shape
    orig = _orig(rows, cols, rows + cols)
    aligns = (1, 512) if cols * 3 % 4 else (512,)   # align 1: rows at any byte, one target per lane (where cols * 3 is a multiple of 4 it changes nothing)
    n = 0
    for name, depth in _maps(rows, cols, rows * 1000 + cols).items():
        images = [(a, up(orig, a), up(depth, 4 if a == 1 else 512)) for a in aligns]
        for view in _views(rows, cols):
            z0 = Z0[n % 3]; n += 1
            want = parallax(orig, depth, *view, z0)
            for align, o, d in images:
                assert_same_image(_run(ctx, o, d, rows, cols, view, z0, align=align), want, (shape, name, align, view, z0))
    at = (cols // 3, rows - 1)
    depth = _maps(rows, cols, 1)["random"]
    o, d = up(orig), up(depth)
    assert_same_image(_run(ctx, o, d, rows, cols, (5, -7, 0.0), at=at), parallax(orig, depth, 5, -7, 0.0, zx=at[0], zy=at[1]), (shape, "pixel form"))


def test_a_whole_row_of_holes_marches_across_the_image(ctx):
    """3 x 500, a far plane, shiftX 256 and dolly 1: ax = 505.5 - x, so every source lands in column 505 or 506, outside; the middle row
    (ay == 0) receives nothing from the other rows either, and each of its holes marches to the right border, then to the left one, and
    keeps the original."""
    rows, cols = 3, 500
    orig = _orig(rows, cols, 1)
    far = np.full((rows, cols), 255.0, np.float32)
    view = (256, 0, 1.0)
    keys, _ = scatter(far, *view, 0.0)
    assert (keys[1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    want = parallax(orig, far, *view, 0.0)
    assert np.array_equal(want[1], orig[1])
    assert_same_image(_run(ctx, up(orig), up(far), rows, cols, view, 0.0), want, "whole row of holes")


def test_ties_go_to_the_smallest_source_index(ctx):
    rows, cols = 61, 83
    orig = _orig(rows, cols, 2)
    const = np.full((rows, cols), 200.0, np.float32)
    for view in ((0, 0, 1.0), (3, -2, 2.5), (0, 0, 0.5)):         # a contracting dolly on a plane behind z0
        _, same = scatter(const, *view, 0.0)
        assert (same >= 2).any(), view                  # at least one target with two or more candidates of equal d': the rule is exercised
        assert_same_image(_run(ctx, up(orig), up(const), rows, cols, view, 0.0), parallax(orig, const, *view, 0.0), view)


@pytest.mark.parametrize("shape", [(5, 97), (9, 300), (4, 2100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_horizontal_case_is_the_stereo_view_on_the_device(ctx, shape):
    rows, cols = shape
    orig = _orig(rows, cols, 3)
    for name, depth in _maps(rows, cols, 77).items():
        o, d = up(orig), up(depth)
        for D in (1, -1, 37, -37, 256, -256):
            for z0 in Z0:
                art = up(np.zeros_like(orig))
                ctx.simulate_stereo(o, d, art, rows, cols, D, z0, -1, -1, rt.STEREO_VIEW)
                ctx.synchronize()
                sv = down(art)
                assert_same_image(_run(ctx, o, d, rows, cols, (D, 0, 0.0), z0), sv, (shape, name, D, z0))
                assert_same_image(sv, stereo(orig, depth, D, z0), "stereo itself")


def test_identities(ctx):
    rows, cols = 61, 83
    orig = _orig(rows, cols, 4)
    depth = _maps(rows, cols, 4)["random"]
    o, d = up(orig), up(depth)
    assert_same_image(_run(ctx, o, d, rows, cols, (0, 0, 0.0), 100.0), orig, "no motion")
    const = np.full((rows, cols), 99.0, np.float32)
    dc = up(const)
    for view in _views(rows, cols):
        assert_same_image(_run(ctx, o, dc, rows, cols, view, 99.0), orig, ("constant map at z0", view))
        assert_same_image(_run(ctx, o, dc, rows, cols, view, at=(5, 6)), orig, ("constant map, pixel form", view))


def test_deterministic_and_independent_of_fp_contraction(ctx):
    rows, cols = 257, 300
    orig = _orig(rows, cols, 5)
    depth = _maps(rows, cols, 5)["random"]
    o, d = up(orig), up(depth)
    view = (-77, 31, _dolly_bound(rows, cols) * 0.5)
    view = (view[0], view[1], float(np.float32(view[2])))
    try:
        outs = []
        for contract in (0, 1, 1):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            outs.append(_run(ctx, o, d, rows, cols, view, 127.5))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    assert_same_image(outs[0], parallax(orig, depth, *view, 127.5), "contraction")


@pytest.mark.parametrize("shape", [(61, 83), (9, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sub_image_views(ctx, shape):
    """Unaligned u8 pointers and pitches, every f32 alignment class of the map: the bytes are the restatement's and no byte outside the
    region of interest of `artistic` changes (Roi.result); the inputs stay as they were."""
    rows, cols = shape
    orig = _orig(rows, cols, 6)
    depth = _maps(rows, cols, 6)["random"]
    view = (-9, 13, float(np.float32(_dolly_bound(rows, cols) * 0.25)))
    want = parallax(orig, depth, *view, 60.0)
    lay_u8 = [(lead, pitch_for(cols * 3, lead, res)) for lead, res in LAYOUTS_U8]
    lay_f32 = [(lead, pitch_for(cols * 4, lead, res)) for lead, res in LAYOUTS_F32]
    ins_o = [Roi(orig, lead, pitch, what="original") for lead, pitch in lay_u8]
    ins_d = [Roi(depth, lead, pitch, what="depth") for lead, pitch in lay_f32]
    for k, (i, j, a) in enumerate(covering(len(lay_u8), len(lay_f32), len(lay_u8))):
        out = Roi(np.zeros_like(orig), *lay_u8[a], FILL_OUTPUT, seed=k, what=f"artistic {lay_u8[a]}")
        ctx.simulate_parallax(ins_o[i].img, ins_d[j].img, out.img, rows, cols, rt.Parallax(*view, 60.0))
        ctx.synchronize()
        assert_same_image(out.result(), want, (shape, lay_u8[i], lay_f32[j], lay_u8[a]))
        ins_o[i].assert_unchanged(); ins_d[j].assert_unchanged()


def test_padding_bytes_stay_untouched(ctx):
    rows, cols, view = 5, 1030, (19, -2, 0.1)
    pitch = cols * 3 + 13
    orig = _orig(rows, cols, 8)
    depth = _maps(rows, cols, 8)["random"]
    base, art = padded_artistic(rows, cols, pitch)
    ctx.simulate_parallax(up(orig), up(depth), art, rows, cols, rt.Parallax(*view, 60.0))
    ctx.synchronize()
    assert_padding_untouched(base, cols)
    assert_same_image(down(art), parallax(orig, depth, *view, 60.0), "padded rows")


def test_the_scratch_is_shared_with_the_defocus_table():
    """A table-path defocus, a parallax (its keys overwrite the table and its zero padding), the same defocus: equal outputs.  Then a
    parallax at another size."""
    rows, cols = 120, 200
    orig = _orig(rows, cols, 9)
    depth = np.random.default_rng(9).uniform(0, 255, (rows, cols)).astype(np.float32)
    with rt.Context(0) as c:
        o, d = up(orig), up(depth)
        c.set_option(rt.OPT_DEFOCUS_PATH, 1)
        outs = []
        for step in range(2):
            art = up(np.zeros_like(orig))
            c.GPUSimulateDefocus(o, d, art, rows, cols)
            c.synchronize()
            assert c.get_option(rt.OPT_DEFOCUS_LAST_PATH) == 1
            outs.append(down(art))
            if step == 0:
                assert_same_image(_run(c, o, d, rows, cols, (40, -25, 0.5), 100.0), parallax(orig, depth, 40, -25, 0.5, 100.0), "between the two defocus calls")
        assert np.array_equal(outs[0], outs[1])
        for r2, c2 in ((37, 91), (300, 260)):           # a smaller image in the same buffer, a larger one in a new one
            o2 = _orig(r2, c2, 10)
            d2 = _maps(r2, c2, 10)["random"]
            assert_same_image(_run(c, up(o2), up(d2), r2, c2, (-11, 17, -0.3), 30.0), parallax(o2, d2, -11, 17, -0.3, 30.0), (r2, c2))
        art = up(np.zeros_like(orig))
        c.GPUSimulateDefocus(o, d, art, rows, cols)
        c.synchronize()
        assert np.array_equal(down(art), outs[0])


def test_pixel_form_reads_the_map_behind_an_unsynchronised_estimate():
    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        view = rt.Parallax(30, -18, 0.05, 0.0, x, y) if value is None else rt.Parallax(30, -18, 0.05, value, -1, -1)
        c.simulate_parallax(o, d, art, rows, cols, view)

    bgr, depth, _, _, fv, image = pixel_form_behind_estimate(call)
    assert_same_image(image, parallax(bgr, depth, 30, -18, 0.05, fv), "pixel form")


def test_parallax_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = _orig(rows, cols, 2)

    def queue(c, o, d, arts):
        c.simulate_parallax(o, d, arts[0], rows, cols, rt.Parallax(31, -14, 0.2, 0.0, 100, 200))
        c.simulate_parallax(o, d, arts[1], rows, cols, rt.Parallax(-12, 0, -0.5, 90.0, -1, -1))

    solved, healed = clean_and_healed(queue, 2, orig)
    assert_same_image(healed[0], parallax(orig, solved, 31, -14, 0.2, zx=100, zy=200), "healed view, pixel form")
    assert_same_image(healed[1], parallax(orig, solved, -12, 0, -0.5, 90.0), "healed view")


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig = _orig(rows, cols, 1)
    depth = _maps(rows, cols, 1)["random"]
    sentinel = np.full_like(orig, 77)
    big = 512.0 / (cols - 1)
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        bad = [dict(shiftX=257), dict(shiftX=-257), dict(shiftY=257), dict(shiftY=-257), dict(shiftX=100000),
               dict(dolly=float("nan")), dict(dolly=float("inf")), dict(dolly=-float("inf")), dict(dolly=big * 1.001), dict(dolly=-big * 1.001),
               dict(zeroParallaxDepth=float("nan")), dict(zeroParallaxDepth=float("inf")), dict(zeroParallaxDepth=-0.5), dict(zeroParallaxDepth=255.5),
               dict(zeroX=cols, zeroY=0), dict(zeroX=0, zeroY=rows), dict(zeroX=5, zeroY=-1), dict(zeroX=cols + 1000, zeroY=rows + 1000)]
        for kw in bad:
            with pytest.raises(rt.RtddError) as e:
                c.simulate_parallax(o, d, art, rows, cols, rt.Parallax(**kw))
            assert e.value.status == 1, kw
        with pytest.raises(rt.RtddError) as e:
            c.simulate_parallax(o, d, art, rows, cols, None)                        # a null view
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_parallax(o, d, o, rows, cols, rt.Parallax(10, 0))            # in place
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_parallax(o, d, art, 0, cols, rt.Parallax(300, 0))            # the parameters are checked before the empty return
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_parallax(o, d, art, 0, cols, None)
        assert e.value.status == 1
        c.simulate_parallax(o, d, o, 0, cols, rt.Parallax(10, 0))                   # ... and the in-place rule after it
        c.simulate_parallax(o, d, o, rows, 0, rt.Parallax(10, 0))
        f = rt.lib().rtdd_simulate_parallax
        assert_bad_images_refused(c, f, o, d, art, rows, cols, (C.byref(rt.Parallax(10, -4, 0.5, 20.0)),))
        po, op, pd, dp, pa, ap = raw_images(o, d, art)
        assert f(c._h, po, op, pd, dp, pa, ap, rows, cols, None) == 1                           # a null view
        for kw in bad:
            w = rt.Parallax(**kw)
            assert f(c._h, po, op, pd, dp, pa, ap, rows, cols, C.byref(w)) == 1, kw
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                                  # nothing was launched
        ok = [dict(shiftX=256, shiftY=-256), dict(shiftX=-256, shiftY=256, zeroParallaxDepth=255.0), dict(dolly=_dolly_bound(rows, cols)),
              dict(dolly=-_dolly_bound(rows, cols)), dict(shiftX=5, zeroX=cols - 1, zeroY=rows - 1), dict(shiftY=5, zeroX=0, zeroY=0),
              dict(zeroParallaxDepth=float("nan"), zeroX=3, zeroY=3)]               # (an unused zeroParallaxDepth is not looked at)
        for kw in ok:                                                               # the bounds themselves are admitted
            c.simulate_parallax(o, d, art, rows, cols, rt.Parallax(**kw))
        c.synchronize()


@pytest.mark.parametrize("args,call", [(["--shift", "19,-11", "--dolly", "0.125", "--zero-parallax", "128"], (19, -11, 0.125, 128.0, -1, -1)),
                                       (["--shift", "-25,0"], (-25, 0, 0.0, 0.0, -1, -1)),
                                       (["--shift", "0,30", "--dolly", "-0.25", "--zero-parallax-at", "300,200"], (0, 30, -0.25, 0.0, 300, 200))])
def test_harness_writes_the_librarys_image(tmp_path, args, call):
    bgr, ann = harness_pair(tmp_path, "pnm")
    rows, cols = bgr.shape[:2]
    got = run_harness(tmp_path, "pnm", ["--effect", "parallax"] + args)[1]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = estimate(c, bgr, ann)
        o, art = up(bgr), up(np.zeros_like(bgr))
        c.simulate_parallax(o, d, art, rows, cols, rt.Parallax(*call))
        c.synchronize()
        want = down(art)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, bgr)


def test_harness_refuses_live_with_parallax():
    r = subprocess.run([harness_bin(), "-i", "unused.ppm", "--live", "3", "--effect", "parallax", "--shift", "10,5"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout
