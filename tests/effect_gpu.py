"""Scaffolding shared by the depth effects' -m gpu tests (tests/test_gpu_{stereo,refocus,lens_blur,relight,relight_shadow,parallax,
ambient_occlusion}.py): the context and the Dog depth map as fixtures, the estimate, image comparison, PNM files, the harness, padded
artistic images, the clean-and-healed pair of solves, the pixel form behind an unsynchronised estimate, and the image refusals of the raw
ABI.  What is particular to an effect -- its inputs, its parameters, its call and its restatement -- stays in its own file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import realtimedepthdiffusion_amd as rt
from dataset_util import load_pair
from gpu_util import down, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "harness", "rtdd_harness")
FILL = 0x5A                 # what an artistic image holds before an effect writes it


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def random_inputs(rows, cols, seed):
    """A random BGR image and a depth map in [-20, 275] with 3 % NaN."""
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    depth = rng.uniform(-20, 275, (rows, cols)).astype(np.float32)
    depth[rng.random((rows, cols)) < 0.03] = np.nan
    return orig, depth


def estimate(c, bgr, ann):
    """Queues one depth estimate of the pair on a fresh pyramid; returns the level-0 depth image (on the device, not synchronised)."""
    rows, cols = bgr.shape[:2]
    c.pyramid_create(rows, cols)
    c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
    c.estimate_depth(1000)
    return c.pyramid_image(rt.IMG_DEPTH, 0)


def tile_mirrored(a, rows, cols):
    """`a` mirrored to the right and downwards, the four-fold tile repeated and cut to rows x cols: no seams."""
    a2 = np.concatenate([a, a[:, ::-1]], 1); a4 = np.concatenate([a2, a2[::-1]], 0)
    return np.ascontiguousarray(np.tile(a4, (-(-rows // a4.shape[0]), -(-cols // a4.shape[1])))[:rows, :cols])


@pytest.fixture(scope="module")
def dog_depth():
    bgr, ann, _ = load_pair("Dog")
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        estimate(c, bgr, ann)
        c.synchronize()
        return c.pyramid_download(rt.IMG_DEPTH, 0)


def assert_same_image(got, want, what):
    """Two rows x cols x 3 u8 images are equal; if not, how many pixels differ."""
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    assert np.array_equal(got, want), f"{what}: {int((got != want).any(-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


def write_pnm(path, a):
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if a.ndim == 3 else b"P5", a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


def read_pnm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip(); w, h = map(int, f.readline().split()); f.readline()
        a = np.frombuffer(f.read(), np.uint8)
    return a.reshape(h, w, 3) if magic == b"P6" else a.reshape(h, w)


def harness_bin():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    return BIN


def _pair_paths(tmp_path, fmt):
    return (tmp_path / "img.png", tmp_path / "ann.png") if fmt == "png" else (tmp_path / "img.ppm", tmp_path / "ann.pgm")


def harness_pair(tmp_path, fmt):
    """Writes the WomanParasol pair into tmp_path as "png" or "pnm" files (RGB, as the harness reads them); returns (bgr, ann)."""
    bgr, ann, _ = load_pair("WomanParasol")
    img_path, ann_path = _pair_paths(tmp_path, fmt)
    if fmt == "png":
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), "RGB").save(img_path)
        Image.fromarray(ann, "L").save(ann_path)
    else:
        write_pnm(img_path, bgr[..., ::-1]); write_pnm(ann_path, ann)
    return bgr, ann


def harness_files(tmp_path, fmt):
    """The harness's -i, -a and -o arguments for the pair that harness_pair(tmp_path, fmt) wrote."""
    img_path, ann_path = _pair_paths(tmp_path, fmt)
    return ["-i", str(img_path), "-a", str(ann_path), "-o", str(tmp_path) + "/"]


def run_harness(tmp_path, fmt, args):
    """Runs the harness on the files of harness_pair(tmp_path, fmt) with `args`; returns (stdout, ArtisticEffect as BGR, DepthMap)."""
    out = subprocess.check_output([harness_bin()] + harness_files(tmp_path, fmt) + (["--png"] if fmt == "png" else []) + args, text=True)
    assert "Saving images" in out
    if fmt == "png":
        from PIL import Image
        return out, np.array(Image.open(tmp_path / "ArtisticEffect.png"))[..., ::-1], np.array(Image.open(tmp_path / "DepthMap.png"))
    return out, read_pnm(tmp_path / "ArtisticEffect.ppm")[..., ::-1], read_pnm(tmp_path / "DepthMap.pgm")


def padded_artistic(rows, cols, pitch, device="cuda:0"):
    """A rows x pitch buffer of FILL bytes and its rows x cols x 3 view, the artistic image: (base, view)."""
    base = torch.full((rows, pitch), FILL, dtype=torch.uint8, device=device)
    return base, base[:, :cols * 3].unflatten(1, (cols, 3))


def assert_padding_untouched(base, cols):
    assert bool((base[:, cols * 3:] == FILL).all()), "padding bytes written"


def clean_and_healed(queue, n_images, orig):
    """Two contexts solve the same synthetic problem of orig's size, the second with a (simulated) time-out status; queue(c, o, d, arts)
    queues the effects behind the solve, unsynchronised, into the n_images artistic images `arts`.  The synchronisation heals the second
    solve once and renders the effects again: depth and images are those of the clean run.  Returns (the clean depth, the healed images)."""
    from realtimedepthdiffusion_amd.synth import make_problem
    rows, cols = orig.shape[:2]
    p = make_problem(rows, cols, seed=6)

    def run(force):
        c = rt.Context(0)
        try:
            c.GPUAllocateDeviceMemory(rows, cols, 1); c.GPULoadWeights(0.4)
            d, m, g = up(p["depth"]), up(p["mask"]), up(p["gray"])
            o = up(orig)
            arts = [up(np.zeros_like(orig)) for _ in range(n_images)]
            if force:
                c.set_option(rt.OPT_DEBUG_FORCE_STATUS, 1)
            c.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, 24, 0.0, 0)
            queue(c, o, d, arts)
            c.synchronize()
            assert c.get_option(rt.OPT_TIMEOUT_HEALS) == (1 if force else 0)
            return [down(d)] + [down(a) for a in arts]
        finally:
            c.close()

    clean, healed = run(False), run(True)
    assert not np.array_equal(clean[0], p["depth"])
    for w, g in zip(clean, healed):
        assert np.array_equal(g, w)
    return clean[0], healed[1:]


def pixel_form_behind_estimate(call):
    """The Dog pair is estimated and a pixel (x, y) in the middle of the depth range chosen; the same estimate is queued again from a cold
    start and call(c, o, d, art, x, y) -- the effect with its depth read at that pixel on the device -- behind it with no synchronisation;
    then call(c, o, d, art, x, y, value=fv) with the value fv that the map holds there.  Equal bytes.  Returns (bgr, depth, x, y, fv, image)."""
    bgr, ann, _ = load_pair("Dog")
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        estimate(c, bgr, ann)
        first = c.pyramid_download(rt.IMG_DEPTH, 0)
        ys, xs = np.nonzero((first > 60) & (first < 200))                 # a pixel in the middle of the depth range
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
        d = estimate(c, bgr, ann)                                           # a new image: the same estimate again, from a cold start
        o = up(bgr)
        a1, a2 = up(np.zeros_like(bgr)), up(np.zeros_like(bgr))
        call(c, o, d, a1, x, y)                                             # no synchronisation since the estimate was queued
        c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
        fv = float(depth[y, x])
        assert 60.0 < fv < 200.0
        call(c, o, d, a2, x, y, value=fv)
        c.synchronize()
        image = down(a1)
        assert np.array_equal(image, down(a2))
    return bgr, depth, x, y, fv, image


def raw_images(o, d, art):
    """The three images as the C ABI takes them: (original, its pitch, depth, its pitch, artistic, its pitch)."""
    return (C.c_void_p(o.data_ptr()), C.c_size_t(o.stride(0)), C.c_void_p(d.data_ptr()), C.c_size_t(d.stride(0) * 4),
            C.c_void_p(art.data_ptr()), C.c_size_t(art.stride(0)))


def assert_bad_images_refused(c, fn, o, d, art, rows, cols, tail):
    """fn, an rtdd_simulate_* of rt.lib() whose arguments end in `tail` (the effect's own, valid), returns RTDD_ERR_INVALID for every bad
    context, image, pitch or size, and `artistic` is the same afterwards: nothing was launched."""
    c.synchronize()
    before = down(art)
    po, op, pd, dp, pa, ap = raw_images(o, d, art)
    short_u8, short_f32 = C.c_size_t(cols * 3 - 1), C.c_size_t(cols * 4 - 4)
    cases = {"null original": (c._h, None, op, pd, dp, pa, ap, rows, cols),
             "null depth": (c._h, po, op, None, dp, pa, ap, rows, cols),
             "null artistic": (c._h, po, op, pd, dp, None, ap, rows, cols),
             "original pitch short of a row": (c._h, po, short_u8, pd, dp, pa, ap, rows, cols),
             "depth pitch short of a row": (c._h, po, op, pd, short_f32, pa, ap, rows, cols),
             "artistic pitch short of a row": (c._h, po, op, pd, dp, pa, short_u8, rows, cols),
             "depth pitch no multiple of 4": (c._h, po, op, pd, C.c_size_t(dp.value + 2), pa, ap, rows, cols),
             "depth pointer off by 2 bytes": (c._h, po, op, C.c_void_p(pd.value + 2), dp, pa, ap, rows, cols),
             "negative rows": (c._h, po, op, pd, dp, pa, ap, -1, cols),
             "rows^2 + cols^2 >= 2^31": (c._h, po, op, pd, dp, pa, ap, 40000, 40000),
             "in place": (c._h, po, op, pd, dp, po, op, rows, cols),
             "null context": (None, po, op, pd, dp, pa, ap, rows, cols)}
    for what, head in cases.items():
        assert fn(*head, *tail) == 1, what
    c.synchronize()
    assert np.array_equal(down(art), before), "a refused call wrote the artistic image"
