"""harness/rtdd_harness --select-grow / --select-shrink / --move-feather end to end (-m gpu): a painted region is grown before it is removed,
and moved with a feathered edge -- against the library's own calls chained by hand through the Python binding on the library's estimate of
the same pair -- and the refusals."""
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from realtimedepthdiffusion_amd import REFINE_FEATHER, REFINE_GROW, REFINE_SHRINK, MaskRefine        # (absent without the feature)
import polygon_ref as pr
from effect_gpu import harness_bin, read_pnm, write_pnm
from gpu_util import down, up
from paint_gpu import ITERS, _pair

pytestmark = pytest.mark.gpu

REGION = [(120, 80), (200, 85), (195, 170), (125, 165)]
REGION_ARGS = ["--regions", "cut", "--region-fill", ";".join(f"{x},{y}" for x, y in REGION) + ":3"]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The pair as files, and a context that holds the library's estimate of it with region 3 painted: (directory, context, bgr)."""
    tmp = tmp_path_factory.mktemp("refine_harness")
    bgr, ann = _pair()                                                       # 336 x 312
    rows, cols = ann.shape
    write_pnm(tmp / "img.ppm", bgr[..., ::-1]); write_pnm(tmp / "ann.pgm", ann)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.pyramid_set_regions(rt.REGION_CUT)
        c.fill_polygon(REGION, pr.constant(3), c.pyramid_image(rt.IMG_REGION_EDITED)[:2], c.pyramid_image(rt.IMG_REGION_MASK)[:2], rows, cols)
        c.estimate_depth(ITERS)
        c.synchronize()
        assert (c.pyramid_download(rt.IMG_REGION_CODE, 0) == 3).sum() > 3000
        yield tmp, c, bgr


def run(tmp, args):
    out = subprocess.check_output([harness_bin(), "-i", str(tmp / "img.ppm"), "-a", str(tmp / "ann.pgm"), "-o", str(tmp) + "/", "--iters", str(ITERS)] + REGION_ARGS + args, text=True)
    assert "Saving images" in out
    return read_pnm(tmp / "ArtisticEffect.ppm")[..., ::-1]


def images(c, bgr):
    rows, cols = bgr.shape[:2]
    new = lambda *shape, dtype=np.uint8: up(np.zeros(shape, dtype))  # noqa: E731
    return rows, cols, up(bgr), c.pyramid_image(rt.IMG_DEPTH, 0)[:2], c.pyramid_image(rt.IMG_REGION_CODE, 0)[:2], new


def test_select_grow_then_remove(scene):
    tmp, c, bgr = scene
    rows, cols, o, d, code, new = images(c, bgr)
    for flag, op, r2 in (("--select-grow", REFINE_GROW, 50), ("--select-shrink", REFINE_SHRINK, 9)):
        mask, art, z = new(rows, cols), new(rows, cols, 3), new(rows, cols, dtype=np.float32)
        c.refine_mask(code, rows, cols, MaskRefine(3, op, r2, r2), mask)
        c.remove_object(o, d, mask, art, z, rows, cols, rt.Removal(0, 0, 20.0))
        c.synchronize()
        m = down(mask)
        assert set(np.unique(m)) == {0, 255} and (m != 0).sum() != (c.pyramid_download(rt.IMG_REGION_CODE, 0) == 3).sum()
        want = down(art)
        assert not np.array_equal(want, bgr)
        assert np.array_equal(run(tmp, ["--remove-region", "3", "--remove-behind", "20", flag, str(r2)]), want), flag


def test_move_feather(scene):
    tmp, c, bgr = scene
    rows, cols, o, d, code, new = images(c, bgr)
    depth = c.pyramid_download(rt.IMG_DEPTH, 0)
    hard = None
    for args, shrink, w, zl in ((["--move-region", "3:-30,12:40", "--move-feather", "3"], 0, 3.0, 40.0), (["--move-region", "3:-30,12:40"], 0, 0.0, 40.0),
                                (["--move-region", "3:10,5", "--select-shrink", "9", "--move-feather", "2.5"], 9, 2.5, None)):
        mask, select = code, 3
        if shrink:
            refined = new(rows, cols)
            c.refine_mask(code, rows, cols, MaskRefine(3, REFINE_SHRINK, shrink, shrink), refined)
            mask, select = refined, 0
        art, z, sprite, moved = new(rows, cols, 3), new(rows, cols, dtype=np.float32), new(rows, cols, 4), new(rows, cols, 3)
        c.remove_object(o, d, mask, art, z, rows, cols, rt.Removal(select, 0, 0.0))          # the removal stays on the hard mask
        if w:
            alpha = new(rows, cols)
            c.refine_mask(mask, rows, cols, MaskRefine(select, REFINE_FEATHER, 0, 0, -w, 0.0), alpha)
            c.lift_layer_matte(o, alpha, rows, cols, 0, 0, sprite, rows, cols)
        else:
            c.lift_layer(o, mask, rows, cols, select, 0, 0, sprite, rows, cols)
        c.synchronize()
        if zl is None:                                                       # its own nearest depth, over the mask the lift read
            zl = float(np.clip(np.nan_to_num(depth[down(mask) != 0]), 0, 255).min())
        dx, dy = (int(v) for v in args[1].split(":")[1].split(","))
        c.composite_layer(art, z, sprite, moved, None, rows, cols, rt.Layer(rows, cols, dx, dy, 256, rt.LAYER_NEAREST, 255, depth0=zl, depth1=zl))
        c.synchronize()
        want = down(moved)
        assert np.array_equal(run(tmp, args), want), args
        if w == 3.0:
            a = down(alpha)
            assert ((a != 0) & (a != 255)).sum() > 300                        # the edge is soft
            soft = want
        elif not shrink:
            hard = want
    assert not np.array_equal(soft, hard)


def test_harness_refuses_a_refinement_it_cannot_do():
    for args, text in ((["--select-grow", "4"], "need --remove-region"), (["--move-feather", "3"], "needs --move-region"),
                       (["--regions", "cut", "--remove-region", "3", "--move-feather", "3"], "needs --move-region"),
                       (["--regions", "cut", "--remove-region", "3", "--select-grow", "4", "--select-shrink", "4"], "one at a time"),
                       (["--regions", "cut", "--remove-region", "3", "--select-grow", "0"], "1..1048576"),
                       (["--regions", "cut", "--move-region", "3:1,1", "--move-feather", "65"], "0 < W <= 64"),
                       (["--regions", "cut", "--move-region", "3:1,1", "--move-feather", "0"], "0 < W <= 64"),
                       (["--live", "3", "--regions", "cut", "--move-region", "3:1,1", "--move-feather", "2"], "not supported with --live or --batch"),
                       (["--batch", "2", "--regions", "cut", "--remove-region", "3", "--select-shrink", "4"], "not supported with --live or --batch")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (args, r.stdout)
