"""harness/rtdd_harness --segment end to end (-m gpu): the surfaces of the harness's own estimate become the regions of the region pair, the
level-0 code plane is filled again, and --remove-region takes one of them out -- against tests/segment_ref.py and tests/remove_ref.py
chained on the library's estimate of the same pair, and the printed counts and records against the restatement's."""
import re
import subprocess

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import regions_ref as rr
import remove_ref as rmr
import segment_ref as sg
from effect_gpu import harness_bin, read_pnm, write_pnm
from gpu_util import up
from paint_gpu import ITERS, _pair

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_harness_segment_then_remove_region(tmp_path):
    bgr, ann = _pair()                                                # 336 x 312
    rows, cols = ann.shape
    write_pnm(tmp_path / "img.ppm", bgr[..., ::-1]); write_pnm(tmp_path / "ann.pgm", ann)
    s = sg.seg(1.0, 0, 200, 150, 6, 3)
    args = [harness_bin(), "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", str(ITERS), "--regions", "cut",
            "--segment", "1,0,200,150,6,3", "--remove-region", "4", "--remove-grow", "2"]
    said = subprocess.check_output(args, text=True)
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(ITERS); c.synchronize()
        depth = c.pyramid_download(rt.IMG_DEPTH, 0)
    ed, mask = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
    lab, info, rec = sg.segment_surfaces(s, ed, mask, depth)
    print(said, info, rec)
    head = re.search(r"segment step 1 band 0,200 minPixels 150: (\d+) components, (\d+) candidates, (\d+) regions, (\d+) pixels", said)
    assert head and tuple(int(v) for v in head.groups()) == info, said
    lines = re.findall(r"segment region (\d+): (\d+) pixels, root (\d+),(\d+), x (\d+)\.\.(\d+), y (\d+)\.\.(\d+), depth (\S+)\.\.(\S+)", said)
    printed = [(int(m[0]), int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[6]), int(m[5]), int(m[7]), int(f32(m[8]).view(np.uint32)), int(f32(m[9]).view(np.uint32)))
               for m in lines]
    assert printed == rec and info[2] >= 2 and (lab == -1).any(), said
    codes = rr.region_codes(ed, mask, 0)
    assert (codes == 4).sum() == rec[1][1] >= 150
    want = rmr.remove(bgr, depth, codes, rmr.removal(4, 2, 0.0))
    assert not np.array_equal(want[0], bgr)
    assert np.array_equal(read_pnm(tmp_path / "ArtisticEffect.ppm")[..., ::-1], want[0])


def test_harness_refuses_segment_where_it_cannot_run():
    for args, text in ((["--segment", "2"], "--segment needs --regions"),
                       (["--regions", "cut", "--live", "3", "--segment", "2"], "--segment is not supported with --live or --batch"),
                       (["--regions", "cut", "--batch", "2", "--segment", "2,0,255"], "--segment is not supported with --live or --batch"),
                       (["--regions", "cut", "--segment", "2,0"], "--segment wants"),
                       (["--regions", "cut", "--segment", "2,0,255,64,8,1,0"], "--segment wants"),
                       (["--regions", "cut", "--segment", "x"], "--segment wants")):
        r = subprocess.run([harness_bin(), "-i", "unused.ppm"] + args, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (args, r.stdout)
