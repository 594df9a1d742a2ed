"""The two-layer parallax view (include/rtdd.h rtdd_simulate_parallax_layered) on the GPU (-m gpu): artistic and coverage byte for byte
and depthOut bit for bit against the numpy restatement of tests/parallax_layers_ref.py -- test_gpu_parallax.py's shapes, maps and views,
no plate, a random plate and a removed blob, every combination of the optional outputs, z0 by value and by pixel; the identities on the
device; the cross-layer tie; a whole row of holes half covered by a plate; determinism and FP contraction; sub-image views of all seven
images; padding; the zero-parallax pixel behind an estimate; the heal log; the host-side refusals; the harness."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from effect_gpu import ctx  # noqa: F401
from effect_gpu import (FILL, assert_same_image, clean_and_healed, estimate, harness_bin, harness_pair, padded_artistic,
                        assert_padding_untouched, pixel_form_behind_estimate, read_pnm, run_harness)
from gpu_util import assert_bit_equal, down, up
from parallax_layers_ref import BACK, FRONT, LEFT, MARCHED, parallax_layers, scatter_layers
from parallax_ref import EMPTY, clamp_depth, parallax
from remove_ref import remove, removal
from roi_util import FILL_OUTPUT, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for
from test_gpu_parallax import SHAPES, Z0, _dolly_bound, _maps, _orig, _views

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = [(z, c) for z in (False, True) for c in (False, True)]        # (depthOut given, coverage given)


def _plates(orig, depth, seed):
    """name -> (plate, plateDepth): none; random colour and depth; the front with a rectangle of other colours and a farther depth."""
    rows, cols = depth.shape
    rng = np.random.default_rng(seed + 100)
    rnd = (rng.integers(0, 256, orig.shape, dtype=np.uint8), rng.uniform(-20, 280, depth.shape).astype(F))
    rnd[1][rng.random(depth.shape) < 0.03] = np.nan
    y0, y1, x0, x1 = rows // 4, max(rows * 3 // 4, rows // 4 + 1), cols // 3, max(cols * 2 // 3, cols // 3 + 1)
    po, pd = orig.copy(), depth.copy()
    po[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    pd[y0:y1, x0:x1] = np.fmin(clamp_depth(depth[y0:y1, x0:x1]) + F(60), F(255))
    return {"none": (None, None), "random": rnd, "removed blob": (po, pd)}


def _run(c, o, d, po, pd, rows, cols, view, z0=0.0, at=None, outs=(True, True), align=512):
    """One call on device images; returns (artistic, depthOut or None, coverage or None) on the host.  The outputs start as FILL bytes."""
    art = up(np.full((rows, cols, 3), FILL, np.uint8), align)
    z = up(np.full((rows, cols), np.nan, F), 4 if align == 1 else align) if outs[0] else None
    cv = up(np.full((rows, cols), FILL, np.uint8), align) if outs[1] else None
    x, y = at if at is not None else (-1, -1)
    c.simulate_parallax_layered(o, d, po, pd, art, z, cv, rows, cols, rt.Parallax(view[0], view[1], view[2], z0, x, y))
    c.synchronize()
    return down(art), down(z) if z is not None else None, down(cv) if cv is not None else None


def _check(got, want, what):
    assert_same_image(got[0], want[0], what)
    if got[1] is not None:
        assert_bit_equal(got[1], want[1], f"{what}: depthOut")
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), f"{what}: {int((got[2] != want[2]).sum())} coverage bytes differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_exact(ctx, shape):
    rows, cols = shape
    orig = _orig(rows, cols, rows + cols)
    aligns = (1, 512) if cols * 3 % 4 else (512,)   # align 1: rows at any byte, one target per lane
    views = _views(rows, cols)
    n = 0
    maps = _maps(rows, cols, rows * 1000 + cols)
    for name in ("random", "disc", "ramp"):
        depth = maps[name]
        for pname, (po, pd) in _plates(orig, depth, n).items():
            images = [(a, up(orig, a), up(depth, 4 if a == 1 else 512), up(po, a) if po is not None else None,
                       up(pd, 4 if a == 1 else 512) if pd is not None else None) for a in aligns]
            for k in range(5):                      # five of the thirteen views per pair, rotating: every view on every shape
                view = views[(5 * n + k) % len(views)]
                z0 = Z0[(n + k) % 3]
                want = parallax_layers(orig, depth, po, pd, *view, z0)
                for align, o, d, p, q in images:
                    for outs in (OUTPUTS[(n + k) % 4], (True, True)):
                        _check(_run(ctx, o, d, p, q, rows, cols, view, z0, outs=outs, align=align), want, (shape, name, pname, align, view, z0, outs))
            n += 1
    at = (cols // 3, rows - 1)                      # the pixel form: the FRONT map's pixel, whatever the plate holds there
    depth = maps["random"]
    po, pd = _plates(orig, depth, 1)["random"]
    want = parallax_layers(orig, depth, po, pd, 5, -7, 0.0, zx=at[0], zy=at[1])
    for outs in OUTPUTS:
        _check(_run(ctx, up(orig), up(depth), up(po), up(pd), rows, cols, (5, -7, 0.0), at=at, outs=outs), want, (shape, "pixel form", outs))


def test_identities_on_the_device(ctx):
    rows, cols = 61, 83
    orig = _orig(rows, cols, 4)
    depth = _maps(rows, cols, 4)["random"]
    other = _orig(rows, cols, 5)
    raw = depth.copy()
    raw[np.isnan(raw)] = -3.0                       # other raw values, the same d'
    o, d = up(orig), up(depth)
    for view in _views(rows, cols)[3:9]:
        single = up(np.zeros_like(orig))
        ctx.simulate_parallax(o, d, single, rows, cols, rt.Parallax(*view, 100.0))
        ctx.synchronize()
        single = down(single)
        bare = _run(ctx, o, d, None, None, rows, cols, view, 100.0)
        assert_same_image(bare[0], single, ("no plate", view))
        assert_same_image(_run(ctx, o, d, None, None, rows, cols, view, 100.0, outs=(False, False))[0], single, ("every optional argument null", view))
        _check(_run(ctx, o, d, o, d, rows, cols, view, 100.0), bare, ("the plate is the front layer", view))
        _check(_run(ctx, o, d, up(orig), up(depth), rows, cols, view, 100.0), bare, ("a copy of the front layer", view))
        _check(_run(ctx, o, d, up(other), up(raw), rows, cols, view, 100.0), bare, ("equal d', other colours", view))
    far = _plates(orig, depth, 1)["removed blob"]
    for po, pd in ((None, None), far):
        art, z, cv = _run(ctx, o, d, up(po) if po is not None else None, up(pd) if pd is not None else None, rows, cols, (0, 0, 0.0), 60.0)
        assert_same_image(art, orig, "no motion")
        assert_bit_equal(z, clamp_depth(depth), "no motion: the front d'")
        assert (cv == FRONT).all()


def test_cross_layer_tie_goes_to_the_front_layer(ctx):
    rows, cols = 61, 83
    rng = np.random.default_rng(4)
    orig, plate = rng.integers(0, 128, (rows, cols, 3), dtype=np.uint8), rng.integers(128, 256, (rows, cols, 3), dtype=np.uint8)
    odd = (np.arange(rows * cols).reshape(rows, cols) & 1) == 1
    depth, pdepth = np.where(odd, 200.0, 255.0).astype(F), np.where(odd, 255.0, 200.0).astype(F)
    for view in ((0, 0, 1.0), (3, -2, 2.5)):
        want = parallax_layers(orig, depth, plate, pdepth, *view, 0.0)
        won200 = (want[1] == F(200)) & np.isin(want[2], (FRONT, BACK))
        assert (won200 & (want[2] == FRONT)).any() and (want[0][won200 & (want[2] == FRONT)] < 128).all()
        _check(_run(ctx, up(orig), up(depth), up(plate), up(pdepth), rows, cols, view, 0.0), want, ("tie", view))


def test_a_whole_row_of_holes_half_covered_by_a_plate(ctx):
    """3 x 500, a far plane, shiftX 256 and dolly 1: no front source lands in the middle row (test_gpu_parallax.py).  The plate holds z0's own
    depth in the left half of that row -- those pixels stay where they are -- and the front's elsewhere: the right half marches left to the
    plate's last pixel."""
    rows, cols = 3, 500
    orig, plate = _orig(rows, cols, 1), _orig(rows, cols, 2)
    far = np.full((rows, cols), 255.0, F)
    pdepth = far.copy()
    pdepth[1, :250] = 0.0
    view = (256, 0, 1.0)
    keys = scatter_layers(far, None, *view, 0.0)
    assert (keys[1] == EMPTY).all()
    want = parallax_layers(orig, far, plate, pdepth, *view, 0.0)
    assert (want[2][1, :250] == BACK).all() and (want[2][1, 250:] == MARCHED).all() and (want[0][1, 250:] == plate[1, 249]).all()
    _check(_run(ctx, up(orig), up(far), up(plate), up(pdepth), rows, cols, view, 0.0), want, "half a row of holes")


def test_deterministic_and_independent_of_fp_contraction(ctx):
    rows, cols = 257, 300
    orig = _orig(rows, cols, 5)
    depth = _maps(rows, cols, 5)["random"]
    po, pd = _plates(orig, depth, 5)["random"]
    o, d, p, q = up(orig), up(depth), up(po), up(pd)
    view = (-77, 31, float(F(_dolly_bound(rows, cols) * 0.5)))
    try:
        outs = []
        for contract in (0, 1, 1):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            outs.append(_run(ctx, o, d, p, q, rows, cols, view, 127.5))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    _check(outs[0], outs[1], "contraction"); _check(outs[1], outs[2], "repeated")
    _check(outs[0], parallax_layers(orig, depth, po, pd, *view, 127.5), "restatement")


@pytest.mark.parametrize("shape", [(61, 83), (9, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sub_image_views(ctx, shape):
    """All seven images inside larger allocations, unaligned u8 pointers and pitches and every f32 alignment class: the results are the
    restatement's, no byte outside the three outputs' regions of interest changes, the four inputs stay as they were."""
    rows, cols = shape
    orig = _orig(rows, cols, 6)
    depth = _maps(rows, cols, 6)["random"]
    po, pd = _plates(orig, depth, 6)["removed blob"]
    view = (-9, 13, float(F(_dolly_bound(rows, cols) * 0.25)))
    want = parallax_layers(orig, depth, po, pd, *view, 60.0)
    lay3 = [(lead, pitch_for(cols * 3, lead, res)) for lead, res in LAYOUTS_U8]
    lay1 = [(lead, pitch_for(cols, lead, res)) for lead, res in LAYOUTS_U8]
    lay4 = [(lead, pitch_for(cols * 4, lead, res)) for lead, res in LAYOUTS_F32]
    ins = [[Roi(orig, *l, what="original") for l in lay3], [Roi(depth, *l, what="depth") for l in lay4],
           [Roi(po, *l, what="plate") for l in lay3], [Roi(pd, *l, what="plateDepth") for l in lay4]]
    for k, idx in enumerate(covering(7, 7, 7, 7, 7, 7, 7)):
        a = Roi(np.zeros_like(orig), *lay3[idx[4]], FILL_OUTPUT, seed=k, what="artistic")
        z = Roi(np.zeros_like(depth), *lay4[idx[5]], FILL_OUTPUT, seed=k + 1, what="depthOut")
        cv = Roi(np.zeros((rows, cols), np.uint8), *lay1[idx[6]], FILL_OUTPUT, seed=k + 2, what="coverage")
        used = [ins[j][idx[j]] for j in range(4)]
        ctx.simulate_parallax_layered(used[0].img, used[1].img, used[2].img, used[3].img, a.img, z.img, cv.img, rows, cols, rt.Parallax(*view, 60.0))
        ctx.synchronize()
        _check((a.result(), z.result(), cv.result()), want, (shape, idx))
        for r in used:
            r.assert_unchanged()


def test_padding_bytes_stay_untouched(ctx):
    import torch
    rows, cols, view = 5, 1030, (19, -2, 0.1)
    orig = _orig(rows, cols, 8)
    depth = _maps(rows, cols, 8)["random"]
    po, pd = _plates(orig, depth, 8)["random"]
    want = parallax_layers(orig, depth, po, pd, *view, 60.0)
    for apitch, zpitch, cpitch in ((cols * 3 + 13, cols * 4 + 20, cols + 7), (cols * 3 + 14, cols * 4 + 16, cols + 6)):   # byte stores; dword and float4 stores
        base, art = padded_artistic(rows, cols, apitch)
        zbase = torch.full((rows, zpitch), FILL, dtype=torch.uint8, device="cuda:0")
        cbase = torch.full((rows, cpitch), FILL, dtype=torch.uint8, device="cuda:0")
        z, cv = (zbase.data_ptr(), zpitch), (cbase.data_ptr(), cpitch)
        ctx.simulate_parallax_layered(up(orig), up(depth), up(po), up(pd), art, z, cv, rows, cols, rt.Parallax(*view, 60.0))
        ctx.synchronize()
        assert_padding_untouched(base, cols)
        assert bool((zbase[:, cols * 4:] == FILL).all()) and bool((cbase[:, cols:] == FILL).all()), "padding bytes written"
        got_z = zbase[:, :cols * 4].contiguous().cpu().numpy().view(F)
        _check((down(art), got_z, cbase[:, :cols].cpu().numpy()), want, ("padded rows", apitch))


def test_pixel_form_reads_the_front_map_behind_an_unsynchronised_estimate():
    state = {}

    def call(c, o, d, art, x, y, value=None):
        rows, cols = o.shape[:2]
        if "plate" not in state:                    # a plate that does not depend on the estimate: the image upside down on a far wall
            bgr = down(o)
            pd = np.full((rows, cols), 250.0, F); pd[:, cols // 2:] = 255.0
            state["host"] = (bgr[::-1].copy(), pd)
            state["plate"] = (up(state["host"][0]), up(pd))
        view = rt.Parallax(30, -18, 0.05, 0.0, x, y) if value is None else rt.Parallax(30, -18, 0.05, value, -1, -1)
        c.simulate_parallax_layered(o, d, *state["plate"], art, None, None, rows, cols, view)

    bgr, depth, _, _, fv, image = pixel_form_behind_estimate(call)
    assert_same_image(image, parallax_layers(bgr, depth, *state["host"], 30, -18, 0.05, fv)[0], "pixel form")


def test_layered_parallax_is_replayed_after_a_healed_solve():
    rows, cols = 270, 480
    orig = _orig(rows, cols, 2)
    plate = _orig(rows, cols, 3)
    pdepth = np.random.default_rng(3).uniform(0, 255, (rows, cols)).astype(F)
    kept = []

    def queue(c, o, d, arts):
        p, q = up(plate), up(pdepth)
        z, cv = up(np.zeros((rows, cols), F)), up(np.zeros((rows, cols), np.uint8))
        kept.append((p, q, z, cv))
        c.simulate_parallax_layered(o, d, p, q, arts[0], z, cv, rows, cols, rt.Parallax(31, -14, 0.2, 0.0, 100, 200))
        c.simulate_parallax_layered(o, d, None, None, arts[1], None, None, rows, cols, rt.Parallax(-12, 0, -0.5, 90.0, -1, -1))

    solved, healed = clean_and_healed(queue, 2, orig)
    want = parallax_layers(orig, solved, plate, pdepth, 31, -14, 0.2, zx=100, zy=200)
    assert_same_image(healed[0], want[0], "healed view, pixel form")
    assert_same_image(healed[1], parallax(orig, solved, -12, 0, -0.5, 90.0), "healed view, no plate")
    _, _, z, cv = kept[-1]                          # the healed context's extra outputs were written again from the healed depth
    assert_bit_equal(down(z), want[1], "healed depthOut")
    assert np.array_equal(down(cv), want[2])


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig = _orig(rows, cols, 1)
    depth = _maps(rows, cols, 1)["random"]
    with rt.Context(0) as c:
        o, d, p, q = up(orig), up(depth), up(orig[::-1].copy()), up(depth[::-1].copy())
        art, z, cv = up(np.full_like(orig, 77)), up(np.full((rows, cols), 7.0, F)), up(np.full((rows, cols), 77, np.uint8))
        f = rt.lib().rtdd_simulate_parallax_layered
        view = rt.Parallax(10, -4, 0.5, 20.0)

        def ptr(t, off=0):
            return C.c_void_p(t.data_ptr() + off)

        def pitch(t):
            return C.c_size_t(t.stride(0) * t.element_size())

        good = dict(ctx=c._h, o=ptr(o), op=pitch(o), d=ptr(d), dp=pitch(d), p=ptr(p), pp=pitch(p), q=ptr(q), qp=pitch(q), a=ptr(art), ap=pitch(art),
                    z=ptr(z), zp=pitch(z), c=ptr(cv), cp=pitch(cv), rows=rows, cols=cols, view=C.byref(view))
        order = ["ctx", "o", "op", "d", "dp", "p", "pp", "q", "qp", "a", "ap", "z", "zp", "c", "cp", "rows", "cols", "view"]

        def call(**kw):
            return f(*[{**good, **kw}[k] for k in order])

        assert call() == 0
        c.synchronize()
        after = (down(art), down(z), down(cv))
        short3, short4 = C.c_size_t(cols * 3 - 1), C.c_size_t(cols * 4 - 4)
        cases = {"null context": dict(ctx=None), "null original": dict(o=None), "null depth": dict(d=None), "null artistic": dict(a=None),
                 "original pitch": dict(op=short3), "depth pitch": dict(dp=short4), "artistic pitch": dict(ap=short3),
                 "depth pitch no multiple of 4": dict(dp=C.c_size_t(good["dp"].value + 2)), "depth pointer off by 2": dict(d=ptr(d, 2)),
                 "negative rows": dict(rows=-1), "too large": dict(rows=40000, cols=40000), "null view": dict(view=None),
                 "plate without its depth": dict(q=None), "plate depth without the plate": dict(p=None),
                 "plate pitch": dict(pp=short3), "plate depth pitch": dict(qp=short4),
                 "plate depth pitch no multiple of 4": dict(qp=C.c_size_t(good["qp"].value + 2)), "plate depth pointer off by 2": dict(q=ptr(q, 2)),
                 "depthOut pitch": dict(zp=short4), "depthOut pitch no multiple of 4": dict(zp=C.c_size_t(good["zp"].value + 2)),
                 "depthOut pointer off by 2": dict(z=ptr(z, 2)), "coverage pitch": dict(cp=C.c_size_t(cols - 1)),
                 "artistic is original": dict(a=good["o"], ap=good["op"]), "artistic is plate": dict(a=good["p"], ap=good["pp"]),
                 "depthOut is depth": dict(z=good["d"], zp=good["dp"]), "depthOut is plateDepth": dict(z=good["q"], zp=good["qp"])}
        for kw in (dict(shiftX=257), dict(shiftY=-257), dict(dolly=float("nan")), dict(dolly=512.0 / (cols - 1) * 1.001),
                   dict(zeroParallaxDepth=255.5), dict(zeroX=cols, zeroY=0), dict(zeroX=5, zeroY=-1)):
            cases[f"view {kw}"] = dict(view=C.byref(rt.Parallax(**kw)))
        for what, kw in cases.items():
            assert call(**kw) == 1, what
        c.synchronize()
        for got, want in zip((down(art), down(z), down(cv)), after):
            assert np.array_equal(got, want), "a refused call wrote an output"
        with pytest.raises(rt.RtddError) as e:
            c.simulate_parallax_layered(o, d, p, None, art, None, None, rows, cols, view)
        assert e.value.status == 1
        assert call(rows=0, view=None) == 1                                         # the view is checked before the empty return
        assert call(rows=0, a=good["o"], ap=good["op"]) == 0                        # ... and the in-place rule after it
        assert call(p=None, q=None, z=None, c=None) == 0                            # every optional argument null
        c.synchronize()


REGION = [(250, 150), (400, 160), (390, 330), (260, 320)]
REGION_ARGS = ["--regions", "cut", "--region-fill", ";".join(f"{x},{y}" for x, y in REGION) + ":3"]


def test_harness_writes_the_librarys_image_depth_and_coverage(tmp_path):
    import polygon_ref as pr
    bgr, ann = harness_pair(tmp_path, "pnm")
    rows, cols = bgr.shape[:2]
    zf, cf = str(tmp_path / "view_depth.pgm"), str(tmp_path / "view_coverage.pgm")
    got = run_harness(tmp_path, "pnm", REGION_ARGS + ["--effect", "parallax", "--shift", "30,-12", "--dolly", "0.05", "--zero-parallax", "128", "--plate-region", "3",
                                                      "--remove-grow", "2", "--remove-behind", "20", "--parallax-depth-out", zf, "--parallax-coverage", cf])[1]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.pyramid_set_regions(rt.REGION_CUT)
        c.fill_polygon(REGION, pr.constant(3), c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], rows, cols)
        c.estimate_depth(1000)
        d, code = c.pyramid_image(rt.IMG_DEPTH, 0), c.pyramid_image(rt.IMG_REGION_CODE, 0)
        o = up(bgr)
        plate, pz = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), F))
        c.remove_object(o, d, code, plate, pz, rows, cols, rt.Removal(3, 2, 20.0))
        art, z, cv, z8 = up(np.zeros_like(bgr)), up(np.zeros((rows, cols), F)), up(np.zeros((rows, cols), np.uint8)), up(np.zeros((rows, cols), np.uint8))
        c.simulate_parallax_layered(o, d, plate, pz, art, z, cv, rows, cols, rt.Parallax(30, -12, 0.05, 128.0))
        zp, zpitch = rt._img(z); up8, u8pitch = rt._img(z8)
        c._check(rt.lib().rtdd_depth_to_u8(c._h, zp, zpitch, up8, u8pitch, C.c_int(rows), C.c_int(cols)))
        c.synchronize()
        want, want_cv, want_z8 = down(art), down(cv), down(z8)
    assert np.array_equal(got, want) and not np.array_equal(want, bgr)
    assert (want_cv == BACK).any()
    assert np.array_equal(read_pnm(cf), want_cv) and np.array_equal(read_pnm(zf), want_z8)


def test_harness_refuses_what_it_cannot_do():
    for args, text in ((["--live", "3", "--regions", "cut", "--effect", "parallax", "--shift", "10,5", "--plate-region", "3"], "not supported with --live"),
                       (["--live", "3", "--parallax-coverage", "c.pgm"], "not supported with --live"),
                       (["--effect", "parallax", "--shift", "1,1", "--plate-region", "3"], "needs --regions"),
                       (["--regions", "cut", "--effect", "haze", "--plate-region", "3"], "need --effect parallax"),
                       (["--regions", "cut", "--effect", "parallax", "--plate-region", "0"], "1..255"),
                       (["--regions", "cut", "--effect", "parallax", "--plate-region", "3", "--remove-region", "3"], "cannot be combined")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (args, r.stdout)
