"""harness/rtdd_harness --wand / --wand-erase / --wand-connect (and, under --live, --wand-at / --wand-erase-at) end to end on a golden
crop, against tests/wand_ref.py and the restated cascade (-m gpu), as tests/test_gpu_harness_fill.py does for --fill / --fill-erase."""
import os
import re
import subprocess

import numpy as np
import pytest

import polygon_ref as pr
import strokes_ref as sr
import wand_ref as wr
from golden_util import NAMES, load
from paint_gpu import _cascade
from test_gpu_harness import BIN, ROOT, _read_pnm, _write_pnm
from test_gpu_harness_fill import _flag as _fill_flag

pytestmark = pytest.mark.gpu


def _flag(wand, frame=None):
    x, y, tol, flags, ax0, ay0, ax1, ay1, l0, l1 = wand
    head = "" if frame is None else f"{frame}:"
    at = "" if frame is None else "-at"
    connect = ["--wand-connect", "8" if flags & wr.WAND_CONNECT_8 else "4"]
    if l0 == wr.STROKE_ERASE:
        return connect + ["--wand-erase" + at, f"{head}{x},{y},{tol}"]
    return connect + ["--wand" + at, f"{head}{x},{y},{tol}" + (f":{l0}" if l0 == l1 else f":{l0},{l1},{ax0},{ay0},{ax1},{ay1}")]


def test_harness_wands_after_the_polygons(tmp_path):
    """--fill, then --wand (a constant label, 4-connected), --wand (a ramp, 8-connected), --wand-erase, in command-line order behind the
    polygon wherever they stand: the map and the annotated image are the restated cascade's, every pixel, and the printed counts the
    restatement's."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[0])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    lasso = ([(100, 0), (160, 0), (160, 20), (100, 20)], pr.constant(90))
    wands = [wr.constant(128, 20, 12, 17),                            # (crosses the lasso: the later call decides)
             (200, 128, 16, wr.WAND_CONNECT_8, 128, 40, 128, 180, 200, 40),
             wr.erase(128, 128, 12)]
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--iters", "200"]
    args += _flag(wands[0]) + _fill_flag(*lasso) + _flag(wands[1]) + _flag(wands[2])
    said = subprocess.check_output(args, text=True)
    oracle, c = _cascade(g)
    before = c.scribble[0].copy()
    assert pr.fill_polygon(*lasso, c.edited[0], c.scribble[0], g["bgr"]) > 1000
    infos = [wr.fill_similar(w, c.edited[0], c.scribble[0], g["bgr"], wr.covered_label) for w in wands]
    assert [i[0] for i in infos] == [int(v) for v in re.findall(r"wand \d+,\d+ tolerance \d+: (\d+) pixels", said)], said
    assert all(i[0] > 500 for i in infos)
    assert ((before != 255) & (c.scribble[0] == 255)).sum() > 5000 and len(np.unique(c.edited[0][c.scribble[0] == 255])) > 60
    assert (c.edited[0][20, 128] == 17).all() and c.scribble[0][128, 128] == 0
    c.estimate(200)
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
    assert np.array_equal(_read_pnm(tmp_path / "DepthMap.pgm"), c.depth_u8)


def test_harness_wands_in_a_live_view(tmp_path):
    """--live 4 with --wand-at / --wand-erase-at: the harness owns the host pair, applies the clicks to it (its own restatement of the
    rule) and asks for the rebuild before the frame that follows an erasing one.  Every frame == the restated cascade."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "harness")])
    g = load(NAMES[1])
    _write_pnm(tmp_path / "img.ppm", g["bgr"][..., ::-1])
    _write_pnm(tmp_path / "ann.pgm", g["annotation"])
    at = {1: [(128, 20, 12, 0, 0, 13, 0, 56, 250, 150)], 2: [wr.erase(128, 20, 20, wr.WAND_CONNECT_8)], 3: [wr.constant(200, 128, 16, 99, wr.WAND_CONNECT_8)]}
    args = [BIN, "-i", str(tmp_path / "img.ppm"), "-a", str(tmp_path / "ann.pgm"), "-o", str(tmp_path) + "/", "--live", "4", "--iters", "200", "--write-all"]
    for f, ws in at.items():
        for w in ws:
            args += _flag(w, f)
    said = subprocess.check_output(args, text=True)
    oracle, c = _cascade(g)
    counts = []
    for n in range(4):
        for w in at.get(n, ()):
            counts.append(wr.fill_similar(w, c.edited[0], c.scribble[0], g["bgr"], wr.covered_label)[0])
        if any(w[8] == wr.STROKE_ERASE for w in at.get(n, ())):
            sr.rebuild(c)
        c.estimate(200)
        assert np.array_equal(_read_pnm(tmp_path / f"DepthMap_{n}.pgm"), c.depth_u8), f"frame {n}"
    assert counts == [int(v) for v in re.findall(r"frame \d+: wand \d+,\d+ tolerance \d+: (\d+) pixels", said)] and min(counts) > 300, said
    assert np.array_equal(_read_pnm(tmp_path / "AnnotatedImage.ppm"), c.edited[0][..., ::-1])
