"""harness/rtdd_harness --region-surface / --surface-global end to end (-m gpu): the regions are clicked on the harness's own estimate, the
level-0 code plane is filled again, and --remove-region takes the clicked region out -- against tests/surface_ref.py and
tests/remove_ref.py chained on the library's estimate of the same pair, and the printed counts and boxes against the restatement's."""
import re
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import remove_ref as rmr
import surface_ref as sf
from effect_gpu import harness_bin, read_pnm, write_pnm
from gpu_util import up
from paint_gpu import ITERS, _pair

pytestmark = pytest.mark.gpu


def test_harness_region_surface_then_remove_region(tmp_path):
    bgr, ann = _pair()                                                # 336 x 312
    rows, cols = ann.shape
    write_pnm(tmp_path / "img.ppm", bgr[..., ::-1]); write_pnm(tmp_path / "ann.pgm", ann)
    clicks = [sf.constant(cols // 2, rows // 2, 2.0, 3, 20, 20), sf.constant(10, 10, 0.0, 7, 3, 3, sf.SURFACE_GLOBAL)]
    args = [harness_bin(), "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", str(ITERS), "--regions", "cut",
            "--region-surface", f"{cols // 2},{rows // 2},2,20,20:3", "--surface-global", "--region-surface", "10,10,0,3,3:7",
            "--remove-region", "3", "--remove-grow", "2"]
    said = subprocess.check_output(args, text=True)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS); c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
    ed, mask = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
    infos = [sf.fill_surface(w, ed, mask, depth, None, sf.covered_graph) for w in clicks]
    printed = [tuple(int(v) for v in m) for m in re.findall(r"region surface \d+,\d+ step \S+ band \S+(?: global)?: region \d+, (\d+) pixels, x (\d+)\.\.(\d+), y (\d+)\.\.(\d+)", said)]
    assert printed == [(n, x0, x1, y0, y1) for n, x0, y0, x1, y1 in infos], said
    assert said.count(" global: region 7") == 1 and infos[0][0] > 200 and infos[1][0] > 200
    codes = np.where(mask == 255, ed[..., 0], 0).astype(np.uint8)
    assert (codes == 3).sum() > 200 and (codes == 7).sum() > 200
    want = rmr.remove(bgr, depth, codes, rmr.removal(3, 2, 0.0))
    assert not np.array_equal(want[0], bgr)
    assert np.array_equal(read_pnm(tmp_path / "ArtisticEffect.ppm")[..., ::-1], want[0])


def test_harness_refuses_region_surface_where_it_cannot_run():
    for args, text in ((["--region-surface", "5,5,2:3"], "needs --regions"),
                       (["--regions", "cut", "--live", "3", "--region-surface", "5,5,2:3"], "not supported with --live or --batch"),
                       (["--regions", "cut", "--batch", "2", "--region-surface", "5,5,2:3"], "not supported with --live or --batch"),
                       (["--regions", "cut", "--region-surface", "5,5,2:0"], "1..255"),
                       (["--regions", "cut", "--region-surface", "5,5:3"], "--region-surface wants")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (args, r.stdout)
