"""harness/rtdd_harness --stroke / --erase and --stroke-at / --erase-at end to end on a golden crop, against tests/strokes_ref.py and the
restated cascade (-m gpu), as tests/test_gpu_harness.py does for --paint."""
import os
import subprocess

import numpy as np
import pytest

import strokes_ref as sr
from golden_util import NAMES, load
from paint_gpu import _cascade, _flag
from test_gpu_harness import BIN, ROOT, _read_pnm, _write_pnm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", [1, 3])
def test_harness_strokes_and_erasures(tmp_path, batch):
    """--paint, then --stroke / --erase in command-line order in ONE rtdd_paint_strokes call: the map and the annotated image are the
    restated cascade's, every pixel; a --batch of three writes the same."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[0])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    paint = (40, 40, 0, 9)
    strokes = [(10, 200, 240, 180, 11, sr.BRUSH_ROUND, 254), (-20, 128, 300, 120, 40, sr.BRUSH_SQUARE, sr.STROKE_ERASE), (100, 100, 160, 140, 7, sr.BRUSH_SQUARE, 64),
               (128, -10, 128, 270, 15, sr.BRUSH_ROUND, sr.STROKE_ERASE), (128, 128, 128, 128, 21, sr.BRUSH_ROUND, 128)]
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", "200", "--paint", "%d,%d,%d,%d" % paint]
    for q in strokes:
        args += _flag(q)
    subprocess.check_output(args + ["--batch", str(batch), "--devices", "1"], text=True)
    oracle, c = _cascade(g)
    before = int((c.scribble[0] == 255).sum())
    oracle.paint_image(*paint, c.edited[0], c.scribble[0])
    sr.paint_strokes(strokes, c.edited[0], c.scribble[0], g["bgr"])
    assert (c.scribble[0][120:130] == 0).mean() > 0.8 and c.scribble[0][128, 128] == 255 and int((c.scribble[0] == 255).sum()) != before
    c.estimate(200)
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
    assert np.array_equal(_read_pnm(tmp_path / "DepthMap.pgm"), c.depth_u8)


def test_harness_strokes_and_an_eraser_in_a_live_view(tmp_path):
    """--live 6 with --stroke-at / --erase-at: the harness owns the host pair, applies the strokes to it and asks for
    rtdd_pyramid_annotation_rebuild before the frame that follows an erase.  Every frame == the restated cascade with the same strokes
    (and the coarse levels zeroed where the harness rebuilt) at the same places in the sequence of warm-started estimates."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[1])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    at = {1: [(30, 40, 90, 70, 9, sr.BRUSH_ROUND, 200)],
          3: [(-10, 130, 270, 126, 60, sr.BRUSH_SQUARE, sr.STROKE_ERASE), (60, 128, 200, 128, 5, sr.BRUSH_ROUND, 32)],
          4: [(200, 20, 220, 240, 13, sr.BRUSH_SQUARE, 10)]}
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--live", "6", "--iters", "200", "--write-all"]
    for f, qs in at.items():
        for q in qs:
            args += _flag(q, f)
    subprocess.check_output(args, text=True)
    oracle, c = _cascade(g)
    _, plain = _cascade(g)
    for n in range(6):
        for q in at.get(n, ()):
            sr.paint_strokes([q], c.edited[0], c.scribble[0], g["bgr"])
            sr.paint_strokes([q], plain.edited[0], plain.scribble[0], g["bgr"])
        if any(q[6] == sr.STROKE_ERASE for q in at.get(n, ())):
            sr.rebuild(c)
        c.estimate(200); plain.estimate(200)
        assert np.array_equal(_read_pnm(tmp_path / f"DepthMap_{n}.pgm"), c.depth_u8), f"frame {n}"
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
    # (the rebuild matters in this sequence: without it the coarse levels keep the erased band's labels)
    assert any((c.scribble[l] != plain.scribble[l]).any() for l in range(1, c.P))
