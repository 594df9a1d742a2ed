"""Depth-aware relighting (include/rtdd.h rtdd_simulate_relight) on the GPU (-m gpu): bit for bit against the numpy restatement of
tests/relight_ref.py, which knows nothing of the kernel -- small and odd shapes and alignments, both kinds of light, lights outside the
image and on the surface, denormal depth differences, NaN and out-of-range depths, 1080p / 4K / 8K; padding bytes; FP contraction; the
anchor pixel read on the device behind an estimate; the heal log; the host-side refusals; the harness.  No tolerance anywhere: every
operation of the header is a correctly rounded IEEE one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import realtimedepthdiffusion_amd as rt
from dataset_util import load_pair
from gpu_util import down, up
from relight_ref import DIRECTIONAL, POINT, light, relight

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "harness", "rtdd_harness")


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def _inputs(rows, cols, seed):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    depth[rng.random((rows, cols)) < 0.03] = np.nan
    return orig, depth


def _relight(c, o, d, rows, cols, L, align=512):
    art = up(np.zeros((rows, cols, 3), np.uint8), align)
    c.simulate_relight(o, d, art, rows, cols, rt.Light(**L))
    c.synchronize()
    return down(art)


def _check(got, want, what):
    assert np.array_equal(got, want), f"{what}: {int((got != want).any(-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


def _lights(rows, cols, relief):
    """Directional and point lights: inside and outside the image, anchored by value and by pixel, coloured, near and far."""
    common = dict(relief=relief, ambient=0.125, diffuse=1.5)
    ax, ay = cols // 3, rows - 1
    return [light(DIRECTIONAL, 0, 0, 1, **common),
            light(DIRECTIONAL, -1, -1, 1, color=(255, 128, 7), **common),
            light(DIRECTIONAL, 3.5, -0.25, 0.015625, **common),
            light(POINT, cols / 2, rows / 2, 10, anchorDepth=100, radius=40, **common),
            light(POINT, -3000.5, rows + 7.25, 2000, anchorDepth=255, radius=5000, color=(10, 200, 255), **common),
            light(POINT, 32767, -32768, 65536, anchorDepth=0, radius=65536, **common),
            light(POINT, ax, ay, 0.5, anchorX=ax, anchorY=ay, radius=3, **common),
            light(POINT, cols + 40.0, 1.0, 25, anchorX=0, anchorY=0, radius=0.001, ambient=0.0, diffuse=8.0, relief=relief)]


@pytest.mark.parametrize("shape,align", [((1, 1), 1), ((1, 37), 1), ((23, 1), 512), ((5, 255), 1), ((7, 257), 4), ((9, 1027), 1),
                                         ((3, 2051), 512), ((6, 1024), 512), ((5, 255), 4), ((9, 1027), 512)])
def test_small_shapes_bit_exact(ctx, shape, align):
    rows, cols = shape
    orig, depth = _inputs(rows, cols, rows * 1000 + cols)
    o, d = up(orig, align), up(depth, align)
    for relief in (0.0, 0.5, 64.0):
        for L in _lights(rows, cols, relief):
            _check(_relight(ctx, o, d, rows, cols, L, align), relight(orig, depth, L), (shape, align, L))


@pytest.mark.parametrize("align", [1, 512])
def test_light_on_the_surface_and_tiny_distances(ctx, align):
    """A point light exactly over a pixel of the surface: vv == 0 there (shade 0), or tiny -- denormal squares under sqrtf and /."""
    rows, cols = 9, 261
    orig, depth = _inputs(rows, cols, 77)
    orig[4, 100:104] = 255
    flat = np.full((rows, cols), 40.0, np.float32)
    o = up(orig, align)
    for name, dm in (("random", depth), ("flat", flat)):
        d = up(dm, align)
        for z in (1e-30, 1e-20, 3e-20, 1e-15, 1e-3):
            for relief in (0.0, 1.0):
                for anchor in (dict(anchorX=101, anchorY=4), dict(anchorDepth=40.0)):
                    L = light(POINT, 101, 4, z, radius=0.5, relief=relief, ambient=0.0, diffuse=8.0, **anchor)
                    _check(_relight(ctx, o, d, rows, cols, L, align), relight(orig, dm, L), (name, z, relief, anchor))


@pytest.mark.parametrize("align", [4, 512])
def test_denormal_depth_differences(ctx, align):
    rows, cols = 8, 519
    rng = np.random.default_rng(3)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    scale = np.array([1e-38, 1e-38, 1e-30, 1e-30, 3e-20, 3e-20, 1e-19, 1.0], np.float32)[:, None]
    depth = (rng.uniform(0, 1, (rows, cols)).astype(np.float32) * scale).astype(np.float32)
    assert (np.abs(np.diff(depth[:2], axis=1)) < 1.2e-38).all()        # f32 denormals
    o, d = up(orig, align), up(depth, align)
    for relief in (0.5, 1.0, 64.0):
        for L in _lights(rows, cols, relief):
            _check(_relight(ctx, o, d, rows, cols, L, align), relight(orig, depth, L), (relief, L))


def test_out_of_range_and_non_finite_depths(ctx):
    rows, cols = 6, 300
    orig, depth = _inputs(rows, cols, 21)
    depth[1, ::7] = np.inf; depth[2, ::5] = -np.inf; depth[3, ::3] = 1e30; depth[4, ::2] = -1e30; depth[5] = np.nan
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 2.0):
        _check(_relight(ctx, o, d, rows, cols, L), relight(orig, depth, L), L)
    L = light(DIRECTIONAL, 1, 2, 3, relief=64, ambient=1.75, diffuse=0)
    want = np.fmin(orig.astype(np.float32) * np.float32(1.75), np.float32(255)).astype(np.int32).astype(np.uint8)
    _check(_relight(ctx, o, d, rows, cols, L), want, "diffuse 0")


def test_identities_on_the_device(ctx):
    rows, cols = 33, 700
    orig, depth = _inputs(rows, cols, 22)
    o = up(orig)
    const = up(np.full((rows, cols), 93.5, np.float32))
    _check(_relight(ctx, o, const, rows, cols, light(DIRECTIONAL, 0, 0, 1, relief=7, ambient=0, diffuse=1)), orig, "the original")
    ramp = np.tile((255 - 0.25 * np.arange(cols)).astype(np.float32), (rows, 1))
    r = up(ramp)
    lit = _relight(ctx, o, r, rows, cols, light(DIRECTIONAL, -1, 0, 1, relief=4, ambient=0, diffuse=1))
    dark = _relight(ctx, o, r, rows, cols, light(DIRECTIONAL, 1, 0, 1, relief=4, ambient=0, diffuse=1))
    assert (dark[:, 1:-1] == 0).all() and lit[:, 1:-1].max() > 100
    d = up(depth)
    of, df = up(np.ascontiguousarray(orig[:, ::-1])), up(np.ascontiguousarray(depth[:, ::-1]))
    common = dict(relief=1.5, ambient=0.125, diffuse=1.0, color=(255, 200, 90))
    a = _relight(ctx, o, d, rows, cols, light(POINT, 40.5, 2.5, 30, anchorX=17, anchorY=3, radius=60, **common))
    b = _relight(ctx, of, df, rows, cols, light(POINT, cols - 1 - 40.5, 2.5, 30, anchorX=cols - 1 - 17, anchorY=3, radius=60, **common))
    _check(b, a[:, ::-1], "mirror")


def _estimate(c, bgr, ann):
    rows, cols = bgr.shape[:2]
    c.pyramid_create(rows, cols)
    c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
    c.estimate_depth(1000)
    return c.pyramid_image(rt.IMG_DEPTH, 0)


def _tile(a, rows, cols):
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


@pytest.fixture(scope="module")
def dog_depth():
    bgr, ann, _ = load_pair("Dog")
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _estimate(c, bgr, ann)
        c.synchronize()
        return c.pyramid_download(rt.IMG_DEPTH, 0)


@pytest.mark.parametrize("rows,cols", [(1080, 1920), (2160, 3840), (4320, 7680)])
def test_full_size(ctx, dog_depth, rows, cols):
    rng = np.random.default_rng(rows)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    random = rng.uniform(0, 255, (rows, cols)).astype(np.float32)
    o = up(orig)
    lights = [light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1.0),
              light(POINT, cols * 0.4, rows * 0.3, 120, anchorX=cols // 2, anchorY=rows // 2, radius=cols / 4, relief=1.5, ambient=0.1, diffuse=3.0,
                    color=(200, 230, 255))]
    for name, depth in (("Dog tiled", _tile(dog_depth, rows, cols)), ("random", random)):
        d = up(depth)
        for L in lights:
            pitch = cols * 3 + 512
            base = torch.full((rows, pitch), 0x5A, dtype=torch.uint8, device="cuda:0")
            art = base[:, :cols * 3].unflatten(1, (cols, 3))
            ctx.simulate_relight(o, d, art, rows, cols, rt.Light(**L))
            ctx.synchronize()
            assert bool((base[:, cols * 3:] == 0x5A).all()), "padding bytes written"
            _check(down(art), relight(orig, depth, L), (rows, name, L["kind"]))


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 5, cols * 3 + 13
    orig, depth = _inputs(rows, cols, 8)
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 1.0)[1:4]:
        base = torch.full((rows, pitch), 0x5A, dtype=torch.uint8, device="cuda:0")
        art = base[:, :cols * 3].unflatten(1, (cols, 3))
        ctx.simulate_relight(o, d, art, rows, cols, rt.Light(**L))
        ctx.synchronize()
        b = base.cpu().numpy()
        assert (b[:, cols * 3:] == 0x5A).all()
        _check(b[:, :cols * 3].reshape(rows, cols, 3), relight(orig, depth, L), L)


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 16, 1500
    orig, depth = _inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    for L in _lights(rows, cols, 3.0):
        try:
            outs = []
            for contract in (0, 1):
                ctx.set_option(rt.OPT_FP_CONTRACT, contract)
                outs.append(_relight(ctx, o, d, rows, cols, L))
        finally:
            ctx.set_option(rt.OPT_FP_CONTRACT, 1)
        assert np.array_equal(outs[0], outs[1])
        _check(outs[0], relight(orig, depth, L), "contraction")


def test_anchor_pixel_is_read_behind_an_unsynchronised_estimate():
    bgr, ann, _ = load_pair("Dog")
    rows, cols = bgr.shape[:2]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _estimate(c, bgr, ann)
        first = c.pyramid_download(rt.IMG_DEPTH, 0)
        ys, xs = np.nonzero((first > 60) & (first < 200))
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
        d = _estimate(c, bgr, ann)                                          # a new image: the same estimate again, from a cold start
        o = up(bgr)
        a1, a2 = up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        L = light(POINT, x, y, 60, anchorX=x, anchorY=y, radius=150, relief=2, ambient=0.2, diffuse=2.0)
        c.simulate_relight(o, d, a1, rows, cols, rt.Light(**L))            # no synchronisation since the estimate was queued
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        fv = float(depth[y, x])
        assert 60.0 < fv < 200.0
        L2 = dict(L, anchorX=-1, anchorY=-1, anchorDepth=fv)
        c.simulate_relight(o, d, a2, rows, cols, rt.Light(**L2))
        c.synchronize()
        assert np.array_equal(down(a1), down(a2))
        _check(down(a1), relight(bgr, depth, L), "pixel form")
        assert not np.array_equal(down(a1), bgr)


def test_relight_is_replayed_after_a_healed_solve():
    from realtimedepthdiffusion_amd.synth import make_problem
    rows, cols = 270, 480
    p = make_problem(rows, cols, seed=6)
    orig = _inputs(rows, cols, 2)[0]
    L1 = light(POINT, 100, 200, 40, anchorX=100, anchorY=200, radius=120, relief=2, ambient=0.2, diffuse=2.0, color=(255, 220, 180))
    L2 = light(DIRECTIONAL, 1, -2, 1.5, relief=3, ambient=0.1, diffuse=1.25)

    def run(force):
        c = rt.Context(0)
        try:
            c.GPUAllocateDeviceMemory(rows, cols, 1); c.GPULoadWeights(0.4)
            d, m, g = up(p["depth"]), up(p["mask"]), up(p["gray"])
            o = up(orig)
            a1, a2 = up(np.zeros_like(orig)), up(np.zeros_like(orig))
            if force:
                c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
            c.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, 24, 0.0, 0)
            light1 = rt.Light(**L1)
            c.simulate_relight(o, d, a1, rows, cols, light1)
            light1.kind, light1.relief, light1.x = 7, -1.0, float("nan")   # the call has read the light: the record holds it by value
            c.simulate_relight(o, d, a2, rows, cols, rt.Light(**L2))
            c.synchronize()
            assert c.get_option(rt.OPT_TIMEOUT_HEALS) == (1 if force else 0)
            return down(d), down(a1), down(a2)
        finally:
            c.close()

    clean, healed = run(False), run(True)
    assert not np.array_equal(clean[0], p["depth"])
    for w, g in zip(clean, healed):
        assert np.array_equal(g, w)
    _check(healed[1], relight(orig, clean[0], L1), "healed point light")
    _check(healed[2], relight(orig, clean[0], L2), "healed directional light")


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = _inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    nan, inf = float("nan"), float("inf")
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        pt = dict(kind=POINT, x=10.0, y=10.0, z=5.0, radius=20.0)
        bad = [dict(kind=2), dict(kind=-1), dict(x=nan), dict(y=inf), dict(z=nan), dict(z=0.0), dict(z=-1.0), dict(anchorDepth=nan), dict(radius=inf),
               dict(relief=nan), dict(relief=-0.5), dict(relief=64.5), dict(ambient=-0.1), dict(ambient=8.5), dict(ambient=nan), dict(diffuse=-0.1),
               dict(diffuse=8.5), dict(diffuse=inf),
               dict(pt, x=-32769.0), dict(pt, x=32768.0), dict(pt, y=-32769.0), dict(pt, y=32768.0), dict(pt, z=65537.0), dict(pt, z=0.0),
               dict(pt, radius=0.0), dict(pt, radius=-1.0), dict(pt, radius=65537.0), dict(pt, radius=nan),
               dict(pt, anchorDepth=-0.5), dict(pt, anchorDepth=255.5), dict(pt, anchorDepth=inf),
               dict(pt, anchorX=cols, anchorY=0), dict(pt, anchorX=0, anchorY=rows), dict(pt, anchorX=5, anchorY=-1),
               dict(pt, anchorX=cols + 1000, anchorY=rows + 1000)]
        for kw in bad:
            with pytest.raises(rt.RtddError) as e:
                c.simulate_relight(o, d, art, rows, cols, rt.Light(**kw))
            assert e.value.status == 1, kw
        with pytest.raises(rt.RtddError) as e:
            c.simulate_relight(o, d, art, rows, cols, None)                     # a null light
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_relight(o, d, o, rows, cols, rt.Light())                 # in place
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_relight(o, d, art, 0, cols, rt.Light(relief=100.0))      # the parameters are checked before the empty return
        assert e.value.status == 1
        c.simulate_relight(o, d, o, 0, cols, rt.Light())                        # ... and the in-place rule after it
        L = rt.lib()
        op, dp, ap = C.c_size_t(o.stride(0)), C.c_size_t(d.stride(0) * 4), C.c_size_t(art.stride(0))
        po, pd, pa = C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(art.data_ptr())
        li = C.byref(rt.Light())
        assert L.rtdd_simulate_relight(c._h, None, op, pd, dp, pa, ap, rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, op, None, dp, pa, ap, rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, op, pd, dp, None, ap, rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, op, pd, dp, pa, C.c_size_t(cols * 3 - 1), rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, C.c_size_t(cols * 3 - 1), pd, dp, pa, ap, rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, op, pd, C.c_size_t(cols * 4 - 4), pa, ap, rows, cols, li) == 1
        assert L.rtdd_simulate_relight(c._h, po, op, pd, dp, pa, ap, 40000, 40000, li) == 1
        assert L.rtdd_simulate_relight(None, po, op, pd, dp, pa, ap, rows, cols, li) == 1
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                             # nothing was launched
        # the bounds themselves are admitted; a directional light ignores the point light's fields but for their finiteness
        for kw in (dict(pt, x=-32768.0, y=32767.0, z=65536.0, radius=65536.0, anchorDepth=255.0), dict(pt, anchorX=cols - 1, anchorY=rows - 1),
                   dict(relief=64.0, ambient=8.0, diffuse=8.0), dict(relief=0.0, ambient=0.0, diffuse=0.0, radius=-5.0, anchorDepth=999.0, anchorX=cols + 5)):
            c.simulate_relight(o, d, art, rows, cols, rt.Light(**kw))
        c.synchronize()
        assert not np.array_equal(down(art), sentinel)


def test_harness_writes_the_restatements_image(tmp_path):
    from PIL import Image
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    bgr, ann, _ = load_pair("WomanParasol")
    rows, cols = bgr.shape[:2]
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), "RGB").save(tmp_path / "img.png")
    Image.fromarray(ann, "L").save(tmp_path / "ann.png")
    with rt.Context(0) as c:                                                   # the harness's own depth map: the same estimate
        c.GPULoadWeights(0.4)
        _estimate(c, bgr, ann)
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        depth_u8 = c.pyramid_download(rt.IMG_DEPTH_U8, 0)
    x, y = 300, 200
    cases = [(["--light-at", f"{x},{y}"],
              light(POINT, x, y, 100, anchorX=x, anchorY=y, radius=200, relief=2, ambient=0.25, diffuse=1)),
             (["--light-at", f"{x},{y}", "--light-height", "40", "--light-radius", "90.5", "--relief", "3", "--ambient", "0.125", "--diffuse", "2.5",
               "--light-color", "120,200,255"],
              light(POINT, x, y, 40, anchorX=x, anchorY=y, radius=90.5, relief=3, ambient=0.125, diffuse=2.5, color=(120, 200, 255))),
             ([], light(DIRECTIONAL, -1, -1, 1, relief=2, ambient=0.25, diffuse=1)),
             (["--light-dir", "2,0.5,1", "--relief", "1"], light(DIRECTIONAL, 2, 0.5, 1, relief=1, ambient=0.25, diffuse=1))]
    for args, L in cases:
        out = subprocess.check_output([BIN, "-i", str(tmp_path / "img.png"), "-a", str(tmp_path / "ann.png"), "-o", str(tmp_path) + "/",
                                       "--effect", "relight", "--png"] + args, text=True)
        assert "Saving images" in out
        assert np.array_equal(np.array(Image.open(tmp_path / "DepthMap.png")), depth_u8)
        got = np.array(Image.open(tmp_path / "ArtisticEffect.png"))[..., ::-1]
        want = relight(bgr, depth, L)
        _check(got, want, args)
        assert (got != bgr).any(-1).mean() > 0.5                               # a visible result


def test_harness_refuses_live_with_relight():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    r = subprocess.run([BIN, "-i", "unused.ppm", "--live", "3", "--effect", "relight"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout
