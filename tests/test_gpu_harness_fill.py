"""harness/rtdd_harness --fill / --fill-erase / --fill-rule end to end on a golden crop, against tests/polygon_ref.py and the restated
cascade (-m gpu), as tests/test_gpu_harness_strokes.py does for --stroke / --erase."""
import os
import subprocess

import numpy as np
import pytest

import polygon_ref as pr
import strokes_ref as sr
from golden_util import NAMES, load
from paint_gpu import _cascade
from paint_gpu import _flag as _stroke_flag
from test_gpu_harness import BIN, ROOT, _read_pnm, _write_pnm

pytestmark = pytest.mark.gpu


def _flag(V, fill):
    pts = ";".join(f"{x},{y}" for x, y in V)
    rule, ax0, ay0, ax1, ay1, l0, l1 = fill
    if l0 == pr.STROKE_ERASE:
        return ["--fill-erase", pts]
    return ["--fill", pts + (f":{l0}" if l0 == l1 else f":{l0},{l1},{ax0},{ay0},{ax1},{ay1}")]


def test_harness_fills_after_the_strokes(tmp_path):
    """--stroke, then --fill (a ramp), --fill-erase, --fill-rule evenodd --fill (a pentagram), in command-line order behind the stroke:
    the map and the annotated image are the restated cascade's, every pixel."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[0])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    rows, cols = g["annotation"].shape
    stroke = (10, 200, 240, 180, 11, sr.BRUSH_ROUND, 254)
    fills = [([(60, 150), (190, 150), (270, 260), (-20, 260)], (pr.FILL_NONZERO, 128, 150, 128, 255, 200, 40)),
             ([(-5, 170), (128, 190), (260, 170), (260, 215), (128, 200), (-5, 215)], pr.erase()),
             (pr.scaled(pr.PENTAGRAM, 4, 3, 40, -10), pr.constant(17, pr.FILL_EVEN_ODD))]
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", "200"]
    args += _flag(*fills[0]) + _stroke_flag(stroke) + _flag(*fills[1]) + ["--fill-rule", "evenodd"] + _flag(*fills[2])     # (the stroke goes first wherever it stands)
    subprocess.check_output(args, text=True)
    oracle, c = _cascade(g)
    before = c.scribble[0].copy()
    sr.paint_strokes([stroke], c.edited[0], c.scribble[0], g["bgr"])
    for V, fill in fills:
        assert pr.fill_polygon(V, fill, c.edited[0], c.scribble[0], g["bgr"]) > 1000
    assert ((before != 255) & (c.scribble[0] == 255)).sum() > 5000 and len(np.unique(c.edited[0][c.scribble[0] == 255])) > 60
    assert c.scribble[0][195, 128] == 0 and c.scribble[0][240, 128] == 255
    nonzero = c.scribble[0].copy()
    pr.fill_polygon(fills[2][0], pr.constant(17), c.edited[0].copy(), nonzero, g["bgr"])
    assert (nonzero != c.scribble[0]).any()                           # (the rule matters: the pentagram's core stays open)
    c.estimate(200)
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
    assert np.array_equal(_read_pnm(tmp_path / "DepthMap.pgm"), c.depth_u8)
