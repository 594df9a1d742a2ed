"""Stereo view and red-cyan anaglyph (include/rtdd.h rtdd_simulate_stereo) on the GPU (-m gpu): bit for bit against the numpy
restatement of tests/stereo_ref.py, which knows nothing of the kernel's segments -- small and odd shapes, adversarial maps at |D| = 256
across segment boundaries, 1080p / 4K / 8K, the widest admitted row; padding bytes; FP contraction; the zero-parallax pixel read on the
device behind an estimate; the heal log; the host-side refusals; the harness."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import realtimedepthdiffusion_amd as rt
from dataset_util import load_pair
from gpu_util import down, up
from stereo_ref import ANAGLYPH, VIEW, stereo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "harness", "rtdd_harness")
DS = [-256, -37, -1, 0, 1, 19, 256]
Z0 = [0.0, 127.5, 255.0]


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


def _stereo(c, o, d, rows, cols, D, z0=0.0, at=None, mode=VIEW, align=512):
    art = up(np.zeros((rows, cols, 3), np.uint8), align)
    x, y = at if at is not None else (-1, -1)
    c.simulate_stereo(o, d, art, rows, cols, D, z0, x, y, mode)
    c.synchronize()
    return down(art)


def _check(got, want, what):
    assert np.array_equal(got, want), f"{what}: {int((got != want).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("shape,align", [((1, 1), 1), ((1, 37), 1), ((23, 1), 512), ((5, 255), 1), ((7, 257), 4), ((4, 300), 512),
                                         ((9, 1027), 1), ((3, 2051), 512)])
def test_small_shapes_bit_exact(ctx, shape, align):
    rows, cols = shape
    orig, depth = _inputs(rows, cols, rows * 1000 + cols)
    o, d = up(orig, align), up(depth, align)
    at = (cols // 3, rows - 1)
    for D in DS:
        for mode in (VIEW, ANAGLYPH):
            for z0 in Z0:
                _check(_stereo(ctx, o, d, rows, cols, D, z0, mode=mode, align=align), stereo(orig, depth, D, z0, mode=mode), (D, z0, mode))
            _check(_stereo(ctx, o, d, rows, cols, D, at=at, mode=mode, align=align), stereo(orig, depth, D, zx=at[0], zy=at[1], mode=mode),
                   (D, "pixel", mode))


def _adversarial(rows, cols, seed):
    """Row groups: per-pixel random depths; 0/255 stripes with widths near 256; a near band one pixel inside a segment boundary."""
    rng = np.random.default_rng(seed)
    depth = np.full((rows, cols), 255.0, np.float32)
    depth[0:4] = rng.uniform(0, 255, (4, cols)).astype(np.float32)
    depth[4:8] = rng.choice([0.0, 255.0], (4, cols)).astype(np.float32)
    for i, w in enumerate((254, 255, 256, 257, 258, 511, 512, 513)):
        r = 8 + i
        x = np.arange(cols)
        depth[r] = np.where((x // w) % 2 == 0, 0.0, 255.0)
    for i, (a, b) in enumerate(((1, 1023), (1025, 1400), (700, 1023), (1025, 1026), (2047, 2049), (0, 1), (cols - 300, cols - 1), (1023, 1025))):
        r = 16 + i
        depth[r, a:b] = 0.0
    return depth


@pytest.mark.parametrize("cols", [3072, 4100])
def test_adversarial_maps_at_the_largest_disparity(ctx, cols):
    rows = 24
    orig = np.random.default_rng(cols).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = _adversarial(rows, cols, cols)
    o, d = up(orig), up(depth)
    for D in (256, -256, 255, -255):
        for z0 in (0.0, 127.5, 255.0):
            _check(_stereo(ctx, o, d, rows, cols, D, z0), stereo(orig, depth, D, z0), (cols, D, z0))
    _check(_stereo(ctx, o, d, rows, cols, 256, mode=ANAGLYPH), stereo(orig, depth, 256, mode=ANAGLYPH), "anaglyph")


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
    orig = np.random.default_rng(rows).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    smooth = (127.5 + 120 * np.sin(xx / 301.0) * np.cos(yy / 207.0)).astype(np.float32)
    o = up(orig)
    for name, depth in (("smooth", smooth), ("Dog tiled", _tile(dog_depth, rows, cols))):
        d = up(depth)
        for D, z0, mode in ((cols // 100, 128.0, VIEW), (-(3 * cols // 100), 64.0, ANAGLYPH), (256, 0.0, VIEW)):
            _check(_stereo(ctx, o, d, rows, cols, D, z0, mode=mode), stereo(orig, depth, D, z0, mode=mode), (rows, name, D))


def test_widest_admitted_row(ctx):
    rows, cols = 3, 46340
    orig, depth = _inputs(rows, cols, 5)
    o, d = up(orig, 1), up(depth, 1)
    for D in (256, -37):
        _check(_stereo(ctx, o, d, rows, cols, D, 100.0, align=1), stereo(orig, depth, D, 100.0), D)


@pytest.mark.parametrize("cols", [37, 1030])
def test_padding_bytes_stay_untouched(ctx, cols):
    rows, pitch = 5, cols * 3 + 13
    orig, depth = _inputs(rows, cols, 8)
    o, d = up(orig), up(depth)
    for mode in (VIEW, ANAGLYPH):
        base = torch.full((rows, pitch), 0x5A, dtype=torch.uint8, device="cuda:0")
        art = base[:, :cols * 3].unflatten(1, (cols, 3))
        ctx.simulate_stereo(o, d, art, rows, cols, 19, 60.0, -1, -1, mode)
        ctx.synchronize()
        b = base.cpu().numpy()
        assert (b[:, cols * 3:] == 0x5A).all()
        _check(b[:, :cols * 3].reshape(rows, cols, 3), stereo(orig, depth, 19, 60.0, mode=mode), mode)


def test_fp_contraction_does_not_change_the_bytes(ctx):
    rows, cols = 16, 1500
    orig, depth = _inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    try:
        outs = []
        for contract in (0, 1):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            outs.append(_stereo(ctx, o, d, rows, cols, -77, 127.5, mode=ANAGLYPH))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1)
    assert np.array_equal(outs[0], outs[1])
    _check(outs[0], stereo(orig, depth, -77, 127.5, mode=ANAGLYPH), "contraction")


def test_pixel_form_reads_the_map_behind_an_unsynchronised_estimate():
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
        c.simulate_stereo(o, d, a1, rows, cols, 40, 0.0, x, y)             # no synchronisation since the estimate was queued
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        fv = float(depth[y, x])
        assert 60.0 < fv < 200.0
        c.simulate_stereo(o, d, a2, rows, cols, 40, fv, -1, -1)
        c.synchronize()
        assert np.array_equal(down(a1), down(a2))
        _check(down(a1), stereo(bgr, depth, 40, fv), "pixel form")


def test_stereo_is_replayed_after_a_healed_solve():
    from realtimedepthdiffusion_amd.synth import make_problem
    rows, cols = 270, 480
    p = make_problem(rows, cols, seed=6)
    orig = _inputs(rows, cols, 2)[0]

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
            c.simulate_stereo(o, d, a1, rows, cols, 31, 0.0, 100, 200)
            c.simulate_stereo(o, d, a2, rows, cols, -12, 90.0, -1, -1, ANAGLYPH)
            c.synchronize()
            assert c.get_option(rt.OPT_TIMEOUT_HEALS) == (1 if force else 0)
            return down(d), down(a1), down(a2)
        finally:
            c.close()

    clean, healed = run(False), run(True)
    assert not np.array_equal(clean[0], p["depth"])
    for w, g in zip(clean, healed):
        assert np.array_equal(g, w)
    _check(clean[1], stereo(orig, clean[0], 31, zx=100, zy=200), "healed view")


def test_invalid_arguments_are_refused_on_the_host():
    rows, cols = 40, 60
    orig, depth = _inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        bad = [dict(D=257), dict(D=-257), dict(D=100000), dict(mode=2), dict(mode=-1),
               dict(z0=float("nan")), dict(z0=float("inf")), dict(z0=-0.5), dict(z0=255.5),
               dict(at=(cols, 0)), dict(at=(0, rows)), dict(at=(5, -1)), dict(at=(cols + 1000, rows + 1000))]
        for kw in bad:
            x, y = kw.get("at", (-1, -1))
            with pytest.raises(rt.RtddError) as e:
                c.simulate_stereo(o, d, art, rows, cols, kw.get("D", 10), kw.get("z0", 0.0), x, y, kw.get("mode", VIEW))
            assert e.value.status == 1, kw
        with pytest.raises(rt.RtddError) as e:
            c.simulate_stereo(o, d, o, rows, cols, 10, 0.0, -1, -1)                 # in place
        assert e.value.status == 1
        with pytest.raises(rt.RtddError) as e:
            c.simulate_stereo(o, d, art, 0, cols, 300, 0.0, -1, -1)                 # the parameters are checked before the empty return
        assert e.value.status == 1
        c.simulate_stereo(o, d, o, 0, cols, 10, 0.0, -1, -1)                        # ... and the in-place rule after it
        L = rt.lib()
        op, dp, ap = C.c_size_t(o.stride(0)), C.c_size_t(d.stride(0) * 4), C.c_size_t(art.stride(0))
        po, pd, pa = C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(art.data_ptr())
        z = C.c_float(0.0)
        assert L.rtdd_simulate_stereo(c._h, None, op, pd, dp, pa, ap, rows, cols, 10, z, -1, -1, 0) == 1
        assert L.rtdd_simulate_stereo(c._h, po, op, pd, dp, pa, C.c_size_t(cols * 3 - 1), rows, cols, 10, z, -1, -1, 0) == 1
        assert L.rtdd_simulate_stereo(c._h, po, op, pd, C.c_size_t(cols * 4 - 4), pa, ap, rows, cols, 10, z, -1, -1, 0) == 1
        assert L.rtdd_simulate_stereo(None, po, op, pd, dp, pa, ap, rows, cols, 10, z, -1, -1, 0) == 1
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                                 # nothing was launched
        for D, z0, at in ((256, 0.0, None), (-256, 255.0, None), (5, 0.0, (cols - 1, rows - 1)), (5, 0.0, (0, 0))):
            x, y = at if at else (-1, -1)
            c.simulate_stereo(o, d, art, rows, cols, D, z0, x, y, ANAGLYPH)
        c.synchronize()


def _write_pnm(path, a):
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if a.ndim == 3 else b"P5", a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


def _read_pnm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip(); w, h = map(int, f.readline().split()); f.readline()
        a = np.frombuffer(f.read(), np.uint8)
    return a.reshape(h, w, 3) if magic == b"P6" else a.reshape(h, w)


@pytest.mark.parametrize("args,call", [(["--disparity", "19", "--zero-parallax", "128"], (19, 128.0, -1, -1, VIEW)),
                                       (["--disparity", "-25", "--anaglyph"], (-25, 0.0, -1, -1, ANAGLYPH)),
                                       (["--disparity", "30", "--zero-parallax-at", "300,200", "--anaglyph"], (30, 0.0, 300, 200, ANAGLYPH))])
def test_harness_writes_the_librarys_image(tmp_path, args, call):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    bgr, ann, _ = load_pair("WomanParasol")
    rows, cols = bgr.shape[:2]
    _write_pnm(tmp_path / "img.ppm", bgr[..., ::-1]); _write_pnm(tmp_path / "ann.pgm", ann)
    out = subprocess.check_output([BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/",
                                   "--effect", "stereo"] + args, text=True)
    assert "Saving images" in out
    got = _read_pnm(tmp_path / "ArtisticEffect.ppm")[..., ::-1]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = _estimate(c, bgr, ann)
        o, art = up(bgr), up(np.zeros_like(bgr))
        c.simulate_stereo(o, d, art, rows, cols, *call)
        c.synchronize()
        want = down(art)
    assert np.array_equal(got, want)


def test_harness_refuses_live_with_stereo():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    r = subprocess.run([BIN, "-i", "unused.ppm", "--live", "3", "--effect", "stereo", "--disparity", "10"], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported with --live" in r.stdout
