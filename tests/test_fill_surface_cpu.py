"""rtdd_fill_surface without a GPU: the restatement the GPU tests compare against (tests/surface_ref.py) is pinned here -- the explicit
queue, scipy's connected components over the link list and the restated tiles with their link carry fill against each other, the carry
fill against iteration on every pair of 10-bit words -- the two scenes that motivate the call and state its limit are solved with the
numpy restatement of the solver and printed, and the header and the Python mirror are checked to declare the call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_restatement as npr
import realtimedepthdiffusion_amd as rt
import surface_ref as sf
import wand_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ROUTES = (sf.covered_queue, sf.covered_graph, lambda d, w: sf.covered_tiled(d, w)[0])


def _agree(depth, wand, what=""):
    want = sf.covered_queue(depth, wand)
    assert want[wand[1], wand[0]], what                               # at least the seed
    assert np.array_equal(sf.covered_graph(depth, wand), want), (what, wand)
    tiled, passes = sf.covered_tiled(depth, wand)
    assert np.array_equal(tiled, want), (what, wand)
    assert passes >= 1 or wand[5] & sf.SURFACE_GLOBAL
    return want


# ---- the link carry fill ---------------------------------------------------------------------------------------------------------------
def test_the_link_fill_is_the_iterated_fill_on_every_pair_of_10_bit_words():
    bits = 10
    h, r = np.meshgrid(np.arange(1 << bits, dtype=np.int64), np.arange(1 << bits, dtype=np.int64), indexing="ij")
    h, r = h.ravel(), r.ravel()
    want = sf.fill_links_naive(h, r, bits)
    got = sf.fill_links_bits(h, r, bits)
    top = (h >> (bits - 1)) & 1 == 1
    assert top.sum() == (~top).sum() == 1 << (2 * bits - 1)
    assert np.array_equal(got[~top], want[~top])                      # the top link bit clear
    assert np.array_equal(got[top], want[top])                        # ... and set: the link into the next word, its carry out dropped
    assert (got & r == r).all() and (got < (1 << bits)).all()
    # a run of links that reaches the top bit, entered from its middle: everything from its foot to bit 9, nothing beyond the word
    assert sf.fill_links_bits(0b1110001110, 0b0010000100, bits) == 0b1110011110 == sf.fill_links_naive(0b1110001110, 0b0010000100, bits)
    # the 64-bit form the tiles use
    rng = np.random.default_rng(1)
    h64 = rng.integers(0, 2 ** 64, 3000, dtype=np.uint64) | rng.integers(0, 2 ** 64, 3000, dtype=np.uint64)
    h64[:4] = [0, 2 ** 64 - 1, 1 << 63, 1]
    r64 = rng.integers(0, 2 ** 64, 3000, dtype=np.uint64) & rng.integers(0, 2 ** 64, 3000, dtype=np.uint64) & rng.integers(0, 2 ** 64, 3000, dtype=np.uint64)
    got = sf.fill_links64(h64, r64)
    for a, b, c in zip(h64.tolist(), r64.tolist(), got.tolist()):
        assert c == sf.fill_links_naive(a, b, 64)


# ---- the three routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [10, 11, 12])
def test_the_three_routes_agree_on_random_fields_and_the_fields_are_not_vacuous(seed):
    sizes = []
    for i, depth, head in sf.random_cases(seed, 0):
        sizes.append(int(_agree(depth, head + (0, 0, 0, 0, 7, 7), f"field {i}").sum()))
        _agree(depth, head[:5] + (sf.SURFACE_GLOBAL, 0, 0, 0, 0, 7, 7), f"field {i}, global")
    print(f"default_rng({seed}): covered sizes {sizes}")
    assert max(sizes) > 67 * 45 // 3 and len(set(sizes)) > 4


def test_the_three_routes_agree_across_word_and_block_borders():
    rows, cols = 150, 200
    rng = np.random.default_rng(30)
    for i, (x, y) in enumerate([(63, 10), (64, 10), (63, 64), (64, 63), (127, 128), (0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)]):
        depth = sf.field(rng, rows, cols)
        below, above = sf.BANDS[i % 6]
        _agree(depth, sf.constant(x, y, sf.STEPS[i % 6], 9, below, above), f"border {i}")


def test_a_two_level_map_gives_the_colour_wands_component():
    """The spiral and the four combs: the depth wand on from_mask(mask) covers what the colour wand covers on wand_ref.from_mask(mask)."""
    rows, cols = 150, 200
    sp = wr.spiral(rows, cols)
    want = wr.covered_queue(wr.from_mask(sp), wr.constant(0, 0, 5, 9))
    assert np.array_equal(want, sp)
    got, passes = sf.covered_tiled(sf.from_mask(sp), sf.constant(0, 0, 4, 9))
    assert np.array_equal(got, want) and np.array_equal(sf.covered_queue(sf.from_mask(sp), sf.constant(0, 0, 4, 9)), want)
    assert np.array_equal(sf.covered_graph(sf.from_mask(sp), sf.constant(0, 0, 4, 9)), want)
    print(f"spiral {rows}x{cols}: {int(sp.sum())} pixels, {passes} Jacobi passes; a round is {rt.WAND_ROUND}")
    assert passes > rt.WAND_ROUND
    for shape in ((150, 200), (37, 150)):
        for d in ("left", "right", "up", "down"):
            cm = wr.comb(*shape, d)
            x, y = wr.comb_seed(*shape, d)
            want = wr.covered_queue(wr.from_mask(cm), wr.constant(x, y, 5, 9))
            assert np.array_equal(want, cm)
            for route in ROUTES:
                assert np.array_equal(route(sf.from_mask(cm), sf.constant(x, y, 4, 9)), want), (shape, d)


def test_what_an_eligibility_plane_cannot_express():
    yy, xx = np.mgrid[:20, :30]
    board = np.where((yy + xx) & 1, f32(104), f32(100)).astype(f32)
    ramp2 = (f32(2) * np.mgrid[:10, :70][1]).astype(f32)
    ramp25 = (f32(2.5) * np.mgrid[:10, :70][1]).astype(f32)
    stairs = (f32(50) + f32(5) * (np.mgrid[:12, :60][1] // 10)).astype(f32)
    for route in ROUTES:
        assert route(board, sf.constant(7, 7, 3, 1)).sum() == 1
        assert route(board, sf.constant(7, 7, 4, 1)).sum() == 600
        m = route(ramp2, sf.constant(35, 3, 2, 1, 10, 10))
        assert m.sum() == 110 and m[:, 30:41].all()                   # depths 60 .. 80: eleven columns
        m = route(ramp25, sf.constant(35, 3, 2, 1, 10, 10))
        assert m.sum() == 10 and m[:, 35].all()                       # the seed's column: no horizontal link at all
        m = route(stairs, sf.constant(25, 5, 3, 1))
        assert m.sum() == 120 and m[:, 20:30].all()                   # one terrace


def test_exact_thresholds():
    row = np.array([[100, 103, np.nextafter(f32(106), f32(np.inf)), 50]], f32)
    for route in ROUTES:
        assert route(row, sf.constant(0, 0, 3, 1)).tolist() == [[True, True, False, False]]
        # the band's edges: d' == lo and d' == hi are admissible, one ulp outside is not
        lo, hi = f32(100) - f32(7), f32(100) + f32(9)
        edge = np.array([[np.nextafter(lo, f32(-np.inf)), lo, 100, hi, np.nextafter(hi, f32(np.inf))]], f32)
        assert route(edge, sf.constant(2, 0, 255, 1, 7, 9)).tolist() == [[False, True, True, True, False]]
        assert route(edge, sf.constant(2, 0, 0, 1, 7, 9, sf.SURFACE_GLOBAL)).tolist() == [[False, True, True, True, False]]


def test_special_values():
    assert sf.clamped(np.array([np.nan, -0.0, -5, 0, 1e-40, 300, np.inf, 255, -np.inf], f32)).tolist() == [0, 0, 0, 0, float(f32(1e-40)), 255, 255, 255, 0]
    assert not np.signbit(sf.clamped(np.array([-0.0, np.nan, -np.inf], f32))).any()
    rows, cols = 30, 70
    depth = sf.special_field(np.random.default_rng(7), rows, cols)
    wand = sf.constant(3, 5, 0, 1, 0, 0)                              # a NaN seed, step = below = above = 0
    m = _agree(depth, wand, "NaN seed")
    assert m[5, 3:8].all() and not m[6, 5] and m.sum() >= 5
    assert (sf.clamped(depth)[m] == 0).all()
    g = _agree(depth, wand[:5] + (sf.SURFACE_GLOBAL,) + wand[6:], "NaN seed, global")
    assert np.array_equal(g, sf.clamped(depth) == 0) and g.sum() > m.sum()
    for x, y, step in ((40, 20, 255), (10, 10, 2.5), (60, 3, 100)):
        _agree(depth, sf.constant(x, y, step, 1), "special")


# ---- the case that motivates the call, and its limit ----------------------------------------------------------------------------------------
def _scene(textured):
    rows, cols = 48, 40
    yy, xx = np.mgrid[:rows, :cols]
    obj = ((yy - 24) / 15) ** 2 + ((xx - 20) / 11) ** 2 <= 1
    assert obj.sum() == 513
    rng = np.random.default_rng(5)
    if textured:                                                      # (the tiles are drawn first, then the noise: 84 .. 150 below)
        tiles = rng.integers(60, 141, (24, 20)).repeat(2, 0).repeat(2, 1)
        gray = np.where(obj, tiles, 200 + rng.integers(-2, 3, (rows, cols)))
    else:
        gray = np.where(obj, np.where(yy < 19, 30, np.where(yy < 29, 120, 230)), 170) + rng.integers(-2, 3, (rows, cols))
    gray = gray.astype(np.uint8)
    e, s = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
    e[12:37, 20] = 60; s[12:37, 20] = 255                             # one stroke across all three parts
    e[1:6, 1:6] = 200; s[1:6, 1:6] = 255                              # one stamp on the background
    depth = np.where(s == 255, e, 128).astype(f32)
    return obj, gray, s, depth


def test_the_depth_wand_selects_what_no_colour_tolerance_does(lut):
    obj, gray, s, depth0 = _scene(False)
    bgr = gray[..., None].repeat(3, -1)
    seed = (20, 24)
    print("selection from (20, 24): covered | missed | background taken")
    hits = []
    for tol in range(256):
        m = wr.covered_queue(bgr, wr.constant(*seed, tol, 1))
        hits.append(np.array_equal(m, obj))
        if tol in (5, 48, 52, 88, 120):
            print(f"  colour wand, tolerance {tol}: {int(m.sum())} | {int((obj & ~m).sum())} | {int((m & ~obj).sum())}")
    assert not any(hits)                                              # no tolerance selects the object
    for sweeps in (300, 1000):
        depth = npr.solve(depth0.copy(), s, gray, sweeps, 0, 0, lut, 1)
        print(f"  after {sweeps} sweeps the depth is {depth[obj].min():.1f} .. {depth[obj].max():.1f} on the object, at least {depth[~obj].min():.1f} outside")
        for what, wand in ([(f"step {k}", sf.constant(*seed, k, 1)) for k in (1, 2, 4, 8)]
                           + [(f"step 255, band {b}", sf.constant(*seed, 255, 1, b, b)) for b in (30, 60)]
                           + [("global, no farther than 30 behind", sf.constant(*seed, 0, 1, 255, 30, sf.SURFACE_GLOBAL))]):
            m = sf.covered_queue(depth, wand)
            print(f"  new rule, {what}: {int(m.sum())} | {int((obj & ~m).sum())} | {int((m & ~obj).sum())}")
            assert np.array_equal(sf.covered_graph(depth, wand), m)
            if what == "step 4":
                assert np.array_equal(m, obj)                         # the three-part object, exactly


def test_a_textured_object_is_the_documented_limit(lut):
    obj, gray, s, depth0 = _scene(True)
    for sweeps in (300, 3000):
        depth = npr.solve(depth0.copy(), s, gray, sweeps, 0, 0, lut, 1)
        for step in (2, 4, 8):
            m = sf.covered_queue(depth, sf.constant(20, 24, step, 1))
            print(f"textured object, {sweeps} sweeps (depth inside {depth[obj].min():.1f} .. {depth[obj].max():.1f}), step {step}: "
                  f"{int((m & obj).sum())} of 513 covered, {int((m & ~obj).sum())} of the background")
            assert (obj & ~m).sum() > 513 // 2                        # a selection is only as good as the depth map


# ---- the writes ------------------------------------------------------------------------------------------------------------------------
def test_the_writes_are_the_lassos():
    import polygon_ref as pr
    rows, cols = 37, 75
    rng = np.random.default_rng(3)
    depth = sf.field(rng, rows, cols)
    orig = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    for kind in (0, 1, 2):
        wand = sf.kinds(40, 20, 2.5, 255, 255, 0, rows, cols)[kind]
        e, s = np.full((rows, cols, 3), 7, np.uint8), np.zeros((rows, cols), np.uint8); s[::3, ::4] = 255
        e0, s0 = e.copy(), s.copy()
        info = sf.fill_surface(wand, e, s, depth, orig if kind == 2 else None)
        m = sf.covered_queue(depth, wand)
        assert info == sf.info_of(m) and 1 < info[0] < rows * cols
        assert np.array_equal(e[~m], e0[~m]) and np.array_equal(s[~m], s0[~m])
        if kind == 2:
            assert np.array_equal(e[m], orig[m]) and (s[m] == 0).all()
        else:
            want = np.array([pr.label_at(x, y, (0,) + wand[6:]) for y, x in zip(*np.nonzero(m))])
            assert (s[m] == 255).all() and np.array_equal(e[m], want[:, None].repeat(3, 1))


# ---- the declarations -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_struct_the_flag_and_the_function():
    header = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    assert "#define RTDD_VERSION 230" in header                     # found by symbol: no version bump
    body = re.search(r"typedef struct rtdd_surface_wand \{(.*?)\} rtdd_surface_wand;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.replace(",", " ").split(";") if d.strip()]
    assert [(d[0], d[1:]) for d in decls] == [("int", ["x", "y"]), ("float", ["step"]), ("float", ["below", "above"]), ("int", ["flags"]),
                                              ("int", ["ax0", "ay0", "ax1", "ay1"]), ("int", ["label0", "label1"])]
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "enum rtdd_surface_flags { RTDD_SURFACE_GLOBAL = 1 };" in code
    assert ("int rtdd_fill_surface(rtdd_ctx *ctx, const rtdd_surface_wand *wand, uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch, "
            "const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch, int rows, int cols, rtdd_wand_info *info );") in code
    assert code.index("int rtdd_fill_similar(") < code.index("enum rtdd_surface_flags") < code.index("int rtdd_fill_surface(") < code.index("int rtdd_simulate_defocus(")
    section = re.sub(r"\s*\n \*\s*", " ", header[header.index("the wand that follows the depth map"):header.index("enum rtdd_surface_flags")])
    for words in ("d > 0 ? fminf(d, 255) : +0", "READ ON THE DEVICE", "lo = ds - below, hi = ds + above", "fabsf(d'(p) - d'(q)) <= step", "nothing wraps",
                  "two more link planes", "THE CALL SYNCHRONISES", "RTDD_ERR_STATE", "NOT deterministic", "only as good as the depth map", "513",
                  "RTDD_REGION_SMOOTH", "is joined to it", "`depth` is never written"):
        assert words in section, words
    assert re.search(r"next bump of RTDD_VERSION should cover rtdd_fill_surface", section)


def test_the_python_wrapper_exposes_them():
    assert [(n, t) for n, t in rt.SurfaceWand._fields_] == [("x", C.c_int), ("y", C.c_int), ("step", C.c_float), ("below", C.c_float), ("above", C.c_float),
                                                            ("flags", C.c_int), ("ax0", C.c_int), ("ay0", C.c_int), ("ax1", C.c_int), ("ay1", C.c_int),
                                                            ("label0", C.c_int), ("label1", C.c_int)]
    assert C.sizeof(rt.SurfaceWand) == 48
    assert rt.SURFACE_GLOBAL == 1 == sf.SURFACE_GLOBAL
    assert "rtdd_fill_surface" in rt.C_ABI_SYMBOLS
    assert callable(rt.Context.fill_surface)
