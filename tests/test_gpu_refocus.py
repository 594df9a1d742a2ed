"""Refocus at a chosen depth and haze with density and airlight (include/rtdd.h rtdd_simulate_refocus, rtdd_simulate_haze_ex) on the
GPU (-m gpu): bit for bit against the restatements of tests/refocus_ref.py and the oracle's literal gather, on both defocus paths, with
column strips and slices; the focus pixel read on the device behind an estimate; the heal log; the host-side refusals; the harness."""
import os
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from dataset_util import PAIRS, load_pair
from effects_ref import effect_inputs
from gpu_util import down, up
from refocus_ref import focus_distance, haze_ex, kernel_size, largest_aperture, refocus_by_summed_area_table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "harness", "rtdd_harness")
FOCI = [0.0, 37.5, 128.0, 255.0]


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def _refocus(c, o, d, rows, cols, aperture=0.025, f=0.0, at=None, path=0):
    """rtdd_simulate_refocus into a fresh artistic image; at = (x, y): the pixel form.  Returns the image on the host."""
    art = up(np.zeros((rows, cols, 3), np.uint8))
    c.set_option(rt.OPT_DEFOCUS_PATH, path)
    try:
        x, y = at if at is not None else (-1, -1)
        c.simulate_refocus(o, d, art, rows, cols, aperture, f, x, y)
        c.synchronize()
    finally:
        c.set_option(rt.OPT_DEFOCUS_PATH, 0)
    return down(art)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("shape,align", [((6, 8), 512), ((23, 37), 1), ((67, 121), 1), ((131, 259), 4), ((270, 480), 512)])
def test_refocus_small_shapes_bit_exact(ctx, shape, align, path):
    rows, cols = shape
    orig, depth = effect_inputs(rows, cols, 31 + rows)
    o, d = up(orig, align), up(depth, align)
    at = (cols // 3, rows - 2)
    for aperture in (0.0, 0.01, 0.025, largest_aperture(rows, cols)):
        for f in FOCI:
            want = refocus_by_summed_area_table(orig, depth, f, aperture)
            assert np.array_equal(_refocus(ctx, o, d, rows, cols, aperture, f, path=path), want), (aperture, f)
        want = refocus_by_summed_area_table(orig, depth, depth[at[1], at[0]], aperture)
        assert np.array_equal(_refocus(ctx, o, d, rows, cols, aperture, at=at, path=path), want), (aperture, "pixel")


@pytest.mark.parametrize("path", [0, 1])
def test_refocus_1080p_against_the_literal_gather(ctx, oracle, path):
    """1080p: the tile kernel (automatic) and the table; every pixel against the oracle's literal gather on |d - f|."""
    rows, cols = 1080, 1920
    orig, depth = effect_inputs(rows, cols, 9)
    o, d = up(orig), up(depth)
    threads = oracle.max_threads()
    got = _refocus(ctx, o, d, rows, cols, f=128.0, path=path)
    assert ctx.get_option(rt.OPT_DEFOCUS_LAST_PATH) == (2 if path == 0 else 1)
    assert np.array_equal(got, oracle.defocus(orig, focus_distance(depth, 128.0), threads=threads))
    at = (1500, 900)
    got = _refocus(ctx, o, d, rows, cols, at=at, path=path)
    assert np.array_equal(got, oracle.defocus(orig, focus_distance(depth, depth[at[1], at[0]]), threads=threads))
    for f in (0.0, 37.5, 255.0):
        assert np.array_equal(_refocus(ctx, o, d, rows, cols, f=f, path=path), refocus_by_summed_area_table(orig, depth, f)), f
    a = largest_aperture(rows, cols)          # K = 255: the tile region does not fit, the table takes it
    assert np.array_equal(_refocus(ctx, o, d, rows, cols, a, 37.5, path=path), refocus_by_summed_area_table(orig, depth, 37.5, a))


@pytest.mark.parametrize("rows,cols,name", [(2160, 3840, "4K"), (4320, 7680, "8K")])
def test_refocus_full_size(ctx, oracle, rows, cols, name):
    """The table path with column strips (automatic at 8K), and banded tables (RTDD_OPT_DEFOCUS_SLICE_MB): every pixel against the
    restatement, sampled pixels against the oracle's literal gather."""
    orig, depth = effect_inputs(rows, cols, 21)
    o, d = up(orig), up(depth)
    rng = np.random.default_rng(3)
    ys = rng.integers(0, rows, 200); xs = rng.integers(0, cols, 200)
    at = (cols // 2 + 7, rows // 2 + 3)
    cases = [(0.025, 128.0, None, 0), (0.025, None, at, 64)]
    if name == "4K":
        cases += [(largest_aperture(rows, cols), 37.5, None, 0), (0.01, 255.0, None, 0)]
    for aperture, f, px, slice_mb in cases:
        ctx.set_option(rt.OPT_DEFOCUS_SLICE_MB, slice_mb)
        try:
            got = _refocus(ctx, o, d, rows, cols, aperture, f if f is not None else 0.0, at=px)
            if slice_mb and name == "8K":
                assert ctx.get_option(rt.OPT_DEFOCUS_LAST_SLICES) > 1
        finally:
            ctx.set_option(rt.OPT_DEFOCUS_SLICE_MB, 0)
        fv = f if f is not None else depth[px[1], px[0]]
        want = refocus_by_summed_area_table(orig, depth, fv, aperture)
        assert np.array_equal(got, want), f"{name} aperture {aperture} f {fv}: {int((got != want).sum())} values differ"
        if aperture == 0.025:
            assert np.array_equal(got[ys, xs], oracle.defocus_at(orig, focus_distance(depth, fv), ys, xs))


def _estimate(c, bgr, ann):
    rows, cols = bgr.shape[:2]
    c.pyramid_create(rows, cols)
    c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
    c.estimate_depth(1000)
    return c.pyramid_image(rt.IMG_DEPTH, 0)


@pytest.mark.parametrize("name", PAIRS)
def test_defaults_equal_defocus_on_the_dataset(name):
    """f = 0, aperture 0.025 is rtdd_simulate_defocus on every pair's estimated depth."""
    bgr, ann, _ = load_pair(name)
    rows, cols = bgr.shape[:2]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = _estimate(c, bgr, ann)
        o = up(bgr)
        a1, a2 = up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        c.GPUSimulateDefocus(o, d, a1, rows, cols)
        c.simulate_refocus(o, d, a2, rows, cols, 0.025, 0.0, -1, -1)
        c.synchronize()
        assert np.array_equal(down(a2), down(a1))


def test_pixel_form_reads_the_map_behind_an_unsynchronised_estimate():
    bgr, ann, _ = load_pair("Dog")
    rows, cols = bgr.shape[:2]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _estimate(c, bgr, ann)
        first = c.pyramid_download(rt.IMG_DEPTH, 0)
        ys, xs = np.nonzero((first > 60) & (first < 200))                 # a pixel in the middle of the depth range
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
        d = _estimate(c, bgr, ann)                                          # a new image: the same estimate again, from a cold start
        o = up(bgr)
        a1, a2 = up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        c.simulate_refocus(o, d, a1, rows, cols, 0.025, 0.0, x, y)          # no synchronisation since the estimate was queued
        c.synchronize()
        fv = float(c.pyramid_download(rt.IMG_DEPTH, 0)[y, x])
        assert 60.0 < fv < 200.0
        c.simulate_refocus(o, d, a2, rows, cols, 0.025, fv, -1, -1)
        c.synchronize()
        assert np.array_equal(down(a1), down(a2))


@pytest.mark.parametrize("align", [512, 1])
def test_haze_ex_at_the_references_constants_is_the_haze(ctx, align):
    rows, cols = 131, 259
    orig, depth = effect_inputs(rows, cols, 4)
    o, d = up(orig, align), up(depth)
    for contract in (1, 0):
        ctx.set_option(rt.OPT_FP_CONTRACT, contract)
        a1, a2 = up(np.zeros_like(orig), align), up(np.zeros_like(orig), align)
        ctx.GPUSimulateHaze(o, d, a1, rows, cols)
        ctx.simulate_haze_ex(o, d, a2, rows, cols, 2.0, (255, 255, 255))
        ctx.synchronize()
        assert np.array_equal(down(a2), down(a1)), contract
    ctx.set_option(rt.OPT_FP_CONTRACT, 1)


@pytest.mark.parametrize("align", [512, 1])
def test_haze_ex_bit_exact_against_the_exact_restatement(ctx, oracle, align):
    rows, cols = 37, 133
    orig, depth = effect_inputs(rows, cols, 6)
    o, d = up(orig, align), up(depth)
    try:
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            for beta, air in ((4.0, (200, 180, 160)), (0.0, (0, 0, 0)), (0.7, (10, 255, 128)), (64.0, (255, 0, 90)), (2.0, (255, 255, 255))):
                art = up(np.zeros_like(orig), align)
                ctx.simulate_haze_ex(o, d, art, rows, cols, beta, air)
                ctx.synchronize()
                want = haze_ex(orig, depth, beta, air, contract, oracle.expf_det)
                assert np.array_equal(down(art), want), (contract, beta, air)
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1)


def test_refocus_and_haze_ex_are_replayed_after_a_healed_solve():
    """A solve with a (simulated) time-out status, refocus (pixel form) and haze_ex queued behind it: the synchronisation heals the
    solve and renders both again from the healed depth -- the images of a clean run."""
    from realtimedepthdiffusion_amd.synth import make_problem
    rows, cols = 270, 480
    p = make_problem(rows, cols, seed=6)
    orig = effect_inputs(rows, cols, 2)[0]

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
            c.simulate_refocus(o, d, a1, rows, cols, 0.025, 0.0, 100, 200)
            c.simulate_haze_ex(o, d, a2, rows, cols, 3.0, (40, 90, 200))
            c.synchronize()
            assert c.get_option(rt.OPT_TIMEOUT_HEALS) == (1 if force else 0)
            return down(d), down(a1), down(a2)
        finally:
            c.close()

    clean, healed = run(False), run(True)
    assert not np.array_equal(clean[0], p["depth"])
    for w, g in zip(clean, healed):
        assert np.array_equal(g, w)


def test_invalid_arguments_are_refused_on_the_host():
    """Every refusal with correctly sized buffers: a refusal that did not happen could never send the GPU through a wild pointer."""
    import ctypes as C
    rows, cols = 40, 60
    orig, depth = effect_inputs(rows, cols, 1)
    sentinel = np.full_like(orig, 77)
    with rt.Context(0) as c:
        o, d, art = up(orig), up(depth), up(sentinel)
        big = 256.5 / float(np.sqrt(np.float32(rows * rows + cols * cols)))
        assert kernel_size(rows, cols, big) == 256
        bad_refocus = [dict(aperture=-0.01), dict(aperture=float("nan")), dict(aperture=float("inf")), dict(aperture=big),
                       dict(f=float("nan")), dict(f=float("inf")), dict(f=-float("inf")),
                       dict(at=(cols, 0)), dict(at=(0, rows)), dict(at=(5, -1)), dict(at=(cols + 1000, rows + 1000))]
        for kw in bad_refocus:
            x, y = kw.get("at", (-1, -1))
            with pytest.raises(rt.RtddError) as e:
                c.simulate_refocus(o, d, art, rows, cols, kw.get("aperture", 0.025), kw.get("f", 0.0), x, y)
            assert e.value.status == 1, kw
        for beta in (float("nan"), float("inf"), -0.5, 64.5, -float("inf")):
            with pytest.raises(rt.RtddError) as e:
                c.simulate_haze_ex(o, d, art, rows, cols, beta, (1, 2, 3))
            assert e.value.status == 1, beta
        with pytest.raises(rt.RtddError) as e:
            c.simulate_refocus(o, d, o, rows, cols, 0.025, 0.0, -1, -1)            # in place
        assert e.value.status == 1
        L = rt.lib()
        op, dp, ap = C.c_size_t(o.stride(0)), C.c_size_t(d.stride(0) * 4), C.c_size_t(art.stride(0))
        po, pd, pa = C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(art.data_ptr())
        f0, a0 = C.c_float(0.0), C.c_double(0.025)
        assert L.rtdd_simulate_refocus(c._h, None, op, pd, dp, pa, ap, rows, cols, a0, f0, -1, -1) == 1
        assert L.rtdd_simulate_refocus(c._h, po, op, pd, dp, pa, C.c_size_t(cols * 3 - 1), rows, cols, a0, f0, -1, -1) == 1
        assert L.rtdd_simulate_haze_ex(c._h, po, op, None, dp, pa, ap, rows, cols, C.c_float(2.0), 1, 2, 3) == 1
        assert L.rtdd_simulate_haze_ex(c._h, po, op, pd, C.c_size_t(cols * 4 - 4), pa, ap, rows, cols, C.c_float(2.0), 1, 2, 3) == 1
        assert L.rtdd_simulate_refocus(None, po, op, pd, dp, pa, ap, rows, cols, a0, f0, -1, -1) == 1
        c.synchronize()
        assert np.array_equal(down(art), sentinel)                            # nothing was launched
        # the limits themselves are accepted
        c.simulate_refocus(o, d, art, rows, cols, largest_aperture(rows, cols), 0.0, cols - 1, rows - 1)
        c.simulate_refocus(o, d, art, rows, cols, 0.0, -1e30, -1, 12345)
        c.simulate_haze_ex(o, d, art, rows, cols, 0.0, (0, 0, 0))
        c.simulate_haze_ex(o, d, art, rows, cols, 64.0, (255, 255, 255))
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


@pytest.mark.parametrize("args", [["--effect", "refocus", "--focus-at", "300,200"],
                                  ["--effect", "refocus", "--focus", "180.5", "--aperture", "0.05"],
                                  ["--effect", "haze", "--haze-beta", "4", "--airlight", "200,180,160"]])
def test_harness_writes_the_librarys_image(tmp_path, args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    bgr, ann, _ = load_pair("WomanParasol")
    rows, cols = bgr.shape[:2]
    _write_pnm(tmp_path / "img.ppm", bgr[..., ::-1]); _write_pnm(tmp_path / "ann.pgm", ann)
    out = subprocess.check_output([BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/"] + args, text=True)
    assert "Saving images" in out
    got = _read_pnm(tmp_path / "ArtisticEffect.ppm")[..., ::-1]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        d = _estimate(c, bgr, ann)
        o, art = up(bgr), up(np.zeros_like(bgr))
        if args[1] == "refocus":
            if args[2] == "--focus-at":
                c.simulate_refocus(o, d, art, rows, cols, 0.025, 0.0, 300, 200)
            else:
                c.simulate_refocus(o, d, art, rows, cols, 0.05, 180.5, -1, -1)
        else:
            c.simulate_haze_ex(o, d, art, rows, cols, 4.0, (200, 180, 160))
        c.synchronize()
        want = down(art)
    assert np.array_equal(got, want)


def test_harness_refuses_live_with_the_aimed_effects(tmp_path):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    for extra in (["--effect", "refocus"], ["--effect", "haze", "--haze-beta", "3"]):
        r = subprocess.run([BIN, "-i", "unused.ppm", "--live", "3"] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "not supported with --live" in r.stdout
