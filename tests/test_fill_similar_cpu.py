"""rtdd_fill_similar without a GPU: the restatement the GPU tests compare against (tests/wand_ref.py) is pinned here -- the explicit
queue, scipy.ndimage.label and the restated tiles with their carry fill against each other, the carry fill against iteration on every
12-bit word, the rule's corner cases -- the case that motivates the feature is solved with the numpy restatement of the solver, and the
header and the Python mirror are checked to declare the call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_restatement as npr
import polygon_ref as pr
import realtimedepthdiffusion_amd as rt
import wand_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows,cols", [(67, 45), (37, 150), (70, 131)])
def test_the_three_routes_agree_on_random_images(rows, cols):
    rng = np.random.default_rng(rows)
    sizes = []
    for i in range(24):
        img = wr.quantised(rng, rows, cols)
        wand = wr.random_wand(rng, rows, cols, 0, (i % 4))            # plain, 8-connected, global, both
        want = wr.covered_queue(img, wand)
        tiled, passes = wr.covered_tiled(img, wand)
        assert np.array_equal(wr.covered_label(img, wand), want), wand
        assert np.array_equal(tiled, want), wand
        assert want[wand[1], wand[0]] and (passes >= 1 or wand[3] & wr.WAND_GLOBAL)
        sizes.append(int(want.sum()))
    assert min(sizes) < 20 and max(sizes) > rows * cols // 2            # single pixels and most of the image are both among them


def test_the_carry_fill_is_the_iterated_fill_on_every_12_bit_word():
    bits = 12
    e, r = np.meshgrid(np.arange(1 << bits, dtype=np.int64), np.arange(1 << bits, dtype=np.int64), indexing="ij")
    sub = (r & ~e) == 0
    e, r = e[sub], r[sub]
    assert len(e) == 3 ** bits                                        # every e with every r inside it
    want = wr.fill_row_naive(e, r, bits)
    assert np.array_equal(wr.fill_row_bits(e, r, bits), want)
    assert (want & ~e == 0).all() and (want & r == r).all()
    assert wr.fill_row_bits(0b011101110111, 0b000100000001, bits) == 0b011100000111 == wr.fill_row_naive(0b011101110111, 0b000100000001, bits)
    # ... and the 64-bit form the tiles use, on words whose runs touch both ends (the carry out of bit 63 is dropped)
    rng = np.random.default_rng(1)
    e64 = rng.integers(0, 2 ** 64, 4000, dtype=np.uint64)
    e64[:4] = [0, 2 ** 64 - 1, 1 << 63, 1]
    r64 = e64 & rng.integers(0, 2 ** 64, 4000, dtype=np.uint64) & rng.integers(0, 2 ** 64, 4000, dtype=np.uint64)
    got = wr.fill_row64(e64, r64)
    for a, b, c in zip(e64.tolist(), r64.tolist(), got.tolist()):
        assert c == wr.fill_row_naive(a, b, 64)


def test_tolerance_0_tolerance_255_and_the_seed():
    rows, cols = 20, 33
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    img[5:9, 10:14] = img[6, 11]                                      # a patch of one colour ...
    img[9, 13] = img[6, 11]; img[9, 13, 1] ^= 1                       # ... and a neighbour one level off in one channel
    for route in (wr.covered_queue, wr.covered_label, lambda o, w: wr.covered_tiled(o, w)[0]):
        m = route(img, wr.constant(11, 6, 0, 7))
        assert m.sum() == 16 and m[5:9, 10:14].all()
        assert route(img, wr.constant(11, 6, 1, 7)).sum() >= 17
        assert route(img, wr.constant(11, 6, 255, 7)).all() and route(img, wr.constant(0, 0, 255, 7, wr.WAND_GLOBAL)).all()
        lone = route(img, wr.constant(30, 2, 0, 7))                   # nothing like it around: the seed alone, always
        assert lone.sum() == 1 and lone[2, 30]
    g = wr.covered_queue(img, wr.constant(11, 6, 0, 7, wr.WAND_GLOBAL))
    img2 = img.copy(); img2[18, 1] = img[6, 11]
    g2 = wr.covered_queue(img2, wr.constant(11, 6, 0, 7, wr.WAND_GLOBAL))
    assert g.sum() == 16 and g2.sum() == 17 and g2[18, 1]             # global: not connected, still covered
    assert wr.info_of(g2) == (17, 1, 5, 13, 18)


def test_a_diagonal_staircase_needs_8_connectivity():
    n = 70                                                            # crosses the block corner (63, 63) -> (64, 64)
    stairs = np.eye(n, dtype=bool)
    img = wr.from_mask(stairs)
    for route in (wr.covered_queue, wr.covered_label, lambda o, w: wr.covered_tiled(o, w)[0]):
        assert route(img, wr.constant(0, 0, 5, 1)).sum() == 1
        assert np.array_equal(route(img, wr.constant(0, 0, 5, 1, wr.WAND_CONNECT_8)), stairs)
        assert np.array_equal(route(img[:, ::-1], wr.constant(n - 1, 0, 5, 1, wr.WAND_CONNECT_8)), stairs[:, ::-1])
    assert wr.covered_tiled(img, wr.constant(0, 0, 5, 1, wr.WAND_CONNECT_8))[1] >= 3      # (one pass per block the stairs enter, and the changeless one)


def test_the_shapes_of_the_gpu_tests_do_what_they_are_for():
    """The spiral is one long path that needs more passes than a round of the host loop; the combs are walked in all four directions."""
    rows, cols = 150, 200
    sp = wr.spiral(rows, cols)
    img = wr.from_mask(sp)
    m, passes = wr.covered_tiled(img, wr.constant(0, 0, 5, 9))
    assert np.array_equal(m, sp) and np.array_equal(wr.covered_queue(img, wr.constant(0, 0, 5, 9)), sp)
    assert 0.45 * rows * cols < sp.sum() < 0.55 * rows * cols
    print(f"spiral {rows}x{cols}: {int(sp.sum())} pixels, {passes} Jacobi passes; a round is {rt.WAND_ROUND}")
    assert passes > 2 * rt.WAND_ROUND
    for d in ("left", "right", "up", "down"):
        cm = wr.comb(37, 150, d)
        x, y = wr.comb_seed(37, 150, d)
        assert cm[y, x]
        got, passes = wr.covered_tiled(wr.from_mask(cm), wr.constant(x, y, 5, 9))
        assert np.array_equal(got, cm) and np.array_equal(wr.covered_label(wr.from_mask(cm), wr.constant(x, y, 5, 9)), cm), d


def test_the_writes_are_the_lassos():
    rows, cols = 37, 75
    rng = np.random.default_rng(3)
    img = wr.quantised(rng, rows, cols)
    for kind in (0, 1, 2):
        wand = wr.random_wand(rng, rows, cols, kind, 0, seed=(40, 20))
        wand = wand[:2] + (12,) + wand[3:]
        e, s = img.copy(), np.zeros((rows, cols), np.uint8); s[::3, ::4] = 255
        e0, s0 = e.copy(), s.copy()
        e[...] = 7; e0[...] = 7
        info = wr.fill_similar(wand, e, s, img)
        m = wr.covered_queue(img, wand)
        assert info == wr.info_of(m) and 1 < info[0] < rows * cols
        assert np.array_equal(e[~m], e0[~m]) and np.array_equal(s[~m], s0[~m])          # uncovered pixels are not written
        if kind == 2:
            assert np.array_equal(e[m], img[m]) and (s[m] == 0).all()
        else:
            want = np.array([pr.label_at(x, y, (0,) + wand[4:]) for y, x in zip(*np.nonzero(m))])
            assert (s[m] == 255).all() and np.array_equal(e[m], want[:, None].repeat(3, 1))
            assert kind == 0 or len(np.unique(want)) > 3


# ---- the case that motivates the feature ----------------------------------------------------------------------------------------------------
def _ellipse_scene(step, seed=5):
    rows, cols = 48, 40
    yy, xx = np.mgrid[:rows, :cols]
    obj = ((yy - 24) / 15) ** 2 + ((xx - 20) / 11) ** 2 <= 1
    assert obj.sum() == 513
    gray = (np.where(obj, 100, 100 + step) + np.random.default_rng(seed).integers(-2, 3, (rows, cols))).astype(np.uint8)
    return obj, gray, gray[..., None].repeat(3, -1)


def test_a_wand_beats_two_stamps_across_a_weak_edge(lut):
    """A 48 x 40 image: an ellipse of 513 pixels, gray 100, on gray 112, both with noise in [-2, 2]; the true depth is 200 on the ellipse and
    40 elsewhere.  Diffusion from a 5 x 5 stamp of each label leaks across the step of 12 gray levels: mean |depth - truth| over the image
    is 63.7 after 300 sweeps of the restated solver and 67.3 after 1000 (this seed).  The two regions selected with tolerance 5 from the
    same two seeds are exactly the ellipse and exactly its complement: 0.0.  Asserted: the wand's error is below half of the stamps' -- a
    comparison, not a tuned threshold."""
    obj, gray, bgr = _ellipse_scene(12)
    rows, cols = gray.shape
    truth = np.where(obj, 200.0, 40.0)
    inside, corner = (20, 24), (3, 3)

    def error(paint, sweeps):
        e, s = np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.uint8)
        paint(e, s)
        depth = np.where(s == 255, e[..., 0], 128).astype(np.float32)
        x = npr.solve(depth, s, gray, sweeps, 0, 0, lut, 1)
        return float(np.abs(x - truth).mean())

    def stamps(e, s):
        for (x, y), label in ((inside, 200), (corner, 40)):
            e[y - 2:y + 3, x - 2:x + 3] = label; s[y - 2:y + 3, x - 2:x + 3] = 255

    def wands(e, s):
        a = wr.fill_similar(wr.constant(*inside, 5, 200), e, s, bgr)
        b = wr.fill_similar(wr.constant(*corner, 5, 40), e, s, bgr)
        assert a[0] == 513 and b[0] == rows * cols - 513

    assert np.array_equal(wr.covered_label(bgr, wr.constant(*inside, 5, 200)), obj)
    assert np.array_equal(wr.covered_label(bgr, wr.constant(*corner, 5, 40)), ~obj)
    for sweeps in (300, 1000):
        by_stamps, by_wand = error(stamps, sweeps), error(wands, sweeps)
        print(f"mean |depth - truth| after {sweeps} sweeps: two 5 x 5 stamps {by_stamps:.1f}, two wand selections {by_wand:.1f}")
        assert by_wand < 0.5 * by_stamps


def test_a_step_within_the_tolerance_leaks():
    """The tool's documented limit: with a step of 8 gray levels and tolerance 5, 102 against 106 is similar and the selection leaves the ellipse."""
    obj, gray, bgr = _ellipse_scene(8)
    m = wr.covered_queue(bgr, wr.constant(20, 24, 5, 200))
    print(f"step 8, tolerance 5: {int(m.sum())} pixels covered, the ellipse has 513")
    assert m.sum() > 513 and (m & ~obj).any()


# ---- the declarations -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_structs_the_flags_and_the_function():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert "#define RTDD_VERSION 230" in header                     # found by symbol: no version bump

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [f.strip() for decl in body.split(";") if decl.strip() for f in decl.replace("int", "", 1).split(",")]

    assert fields("rtdd_wand") == ["x", "y", "tolerance", "flags", "ax0", "ay0", "ax1", "ay1", "label0", "label1"]
    assert fields("rtdd_wand_info") == ["pixels", "x0", "y0", "x1", "y1", "passes"]
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "enum rtdd_wand_flags { RTDD_WAND_CONNECT_8 = 1, RTDD_WAND_GLOBAL = 2 };" in code
    assert ("int rtdd_fill_similar(rtdd_ctx *ctx, const rtdd_wand *wand, uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch, "
            "const uint8_t *original, size_t originalPitch, int rows, int cols, rtdd_wand_info *info );") in code
    assert code.index("int rtdd_fill_polygon(") < code.index("enum rtdd_wand_flags") < code.index("int rtdd_fill_similar(") < code.index("int rtdd_simulate_defocus(")
    section = re.sub(r"\s*\n \*\s*", " ", header[header.index("the magic wand"):header.index("enum rtdd_wand_flags")])
    for words in ("max(|B - sB|, |G - sG|, |R - sR|) <= tolerance", "READ ON THE DEVICE", "RTDD_WAND_GLOBAL every eligible pixel", "nothing wraps",
                  "t = min(max(v.d, 0), dd)", "L = N / (2 * dd)", "THE CALL SYNCHRONISES", "rows == 0 or cols == 0 is", "RTDD_ERR_STATE", "NOT deterministic"):
        assert words in section, words
    assert re.search(r"next bump of RTDD_VERSION should cover rtdd_fill_similar", section)


def test_the_python_wrapper_exposes_them():
    assert [n for n, _ in rt.Wand._fields_] == ["x", "y", "tolerance", "flags", "ax0", "ay0", "ax1", "ay1", "label0", "label1"]
    assert [n for n, _ in rt.WandInfo._fields_] == ["pixels", "x0", "y0", "x1", "y1", "passes"]
    assert all(t is C.c_int for _, t in rt.Wand._fields_ + rt.WandInfo._fields_)
    assert C.sizeof(rt.Wand) == 40 and C.sizeof(rt.WandInfo) == 24
    assert (rt.WAND_CONNECT_8, rt.WAND_GLOBAL) == (1, 2) == (wr.WAND_CONNECT_8, wr.WAND_GLOBAL)
    assert "rtdd_fill_similar" in rt.C_ABI_SYMBOLS
    assert callable(rt.Context.fill_similar)
    source = open(os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "fill_similar.hip")).read()
    assert int(re.search(r"constexpr int kWandRound = (\d+);", source).group(1)) == rt.WAND_ROUND
