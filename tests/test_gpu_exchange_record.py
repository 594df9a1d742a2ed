"""The persistent Jacobi sweep's halo exchange addressed through its per-thread exchange record (csrc/sweep_blocked.hip `xrec`:
32-bit plane offsets, store / load bits per row, the straddle bit) on the smallest shapes at which that addressing can go wrong
(-m gpu; tests/exchange_shapes.py, covered without a GPU by tests/test_exchange_shapes_cpu.py).  Every solve must run as ONE persistent
launch with the asked tile and depth and give the oracle's bits; no tolerance anywhere."""
import pytest

import exchange_shapes as xs
import realtimedepthdiffusion_amd as rt
import tile_geometry as tg
from cascade_ref import Cascade, pyramid_levels
from gpu_util import down, up
from roi_util import FILL_OUTPUT, Roi
from test_gpu_batch import _compare
from test_gpu_cascade import _bgr
from test_gpu_tile_geometry import Failures, _defaults, _problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    _defaults(c)
    yield c
    c.close()


def _fix(c, tile, T, contract=1):
    c.set_option(rt.OPT_FP_CONTRACT, contract); c.set_option(rt.OPT_PERSISTENT, 1)
    c.set_option(rt.OPT_SWEEP_KERNEL, 2); c.set_option(rt.OPT_TILE, tile); c.set_option(rt.OPT_TEMPORAL_DEPTH, T)


_wanted = {}


def _want(oracle, lut, case, contract):
    """The oracle's result of a case, computed once and shared."""
    key = (case.rows, case.cols, case.n, contract)
    if key not in _wanted:
        p = _problem(case.rows, case.cols)
        _wanted[key] = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], case.n, 0, 0, lut, contract, threads=min(8, oracle.max_threads()))
    return _wanted[key]


def _solve(ctx, fails, case, contract, want, images=None):
    p = _problem(case.rows, case.cols)
    what = f"tile {case.tile} depth {case.T} {case.rows}x{case.cols} [{case.tag}] x{case.n} contract {contract}"
    ctx.GPUAllocateDeviceMemory(case.rows, case.cols, 1)
    _fix(ctx, case.tile, case.T, contract)
    for rep in range(2):                     # (the hand-off flags are epoch based and never reset: a second run meets what the first left)
        d, m, g = images(p) if images else (up(p["depth"]), up(p["mask"]), up(p["gray"]))
        ctx.GPUMatrixFreeSolver(getattr(d, "img", d), getattr(m, "img", m), getattr(g, "img", g), case.rows, case.cols, 0.4, case.n, 0.0, 0)
        ctx.synchronize()
        info = ctx.last_solve_info()
        path = (info.kernel, info.tile, info.persistent, info.temporal_depth, info.launches, info.iterations)
        fails.expect(path == (2, case.tile, 1, case.T, 1, case.n), f"{what} rep {rep}: ran (kernel, tile, persistent, depth, launches, sweeps) = {path} [{info.describe()}]")
        fails.check(d.result() if images else down(d), want, f"{what} rep {rep}")
        if images:
            m.assert_unchanged(); g.assert_unchanged()
    fails.cases += 1


@pytest.mark.parametrize("tile", xs.TILES)
def test_exchange_record_on_both_paths(ctx, oracle, lut, tile):
    """Tiles 4, 6 and 9 (LX 32 and 16, G 3 and 1) at depths 4 and 8 on a 3 x 3 grid with a ragged last tile row: a width of
    2*TW + hx + 1 (cols % 4 == 1: the last tile column loads groups across the image's edge -- the select path -- while the other
    columns' waves take the common one) and of 3*TW (no select anywhere); 2*T + 3 and 3*T sweeps (both exchange-buffer parities, with
    and without a tail block)."""
    fails = Failures()
    try:
        for case in xs.cases(tile):
            _solve(ctx, fails, case, 1, _want(oracle, lut, case, 1))
    finally:
        _defaults(ctx)
    fails.expect(ctx.get_option(rt.OPT_TIMEOUT_HEALS) == 0, f"{ctx.get_option(rt.OPT_TIMEOUT_HEALS)} persistent launches timed out and were healed")
    fails.done()


@pytest.mark.parametrize("contract", [1, 0])
def test_exchange_record_with_and_without_contraction(ctx, oracle, lut, contract):
    """OPT_FP_CONTRACT both ways (the two instantiations of every tile) on the straddling shape of tile 6 at depth 8."""
    case = next(c for c in xs.cases(6) if c.T == 8 and c.tag == "straddle" and c.n == 2 * 8 + 3)
    fails = Failures()
    try:
        _solve(ctx, fails, case, contract, _want(oracle, lut, case, contract))
    finally:
        _defaults(ctx)
    fails.done()


def test_exchange_record_on_a_sub_image_view(ctx, oracle, lut):
    """The caller's images are views into larger allocations, their pitch larger than their width: the record's offsets are relative to
    the library's own planes, whatever the caller's layout, and nothing outside the views is written."""
    case = next(c for c in xs.cases(6) if c.T == 8 and c.tag == "straddle" and c.n == 3 * 8)

    def views(p):
        return (Roi(p["depth"], 4, case.cols * 4 + 3 * 64 + 4, FILL_OUTPUT, seed=11, what="depth"), Roi(p["mask"], 3, case.cols + 77, what="scribble"),
                Roi(p["gray"], 1, case.cols + 130, what="gray"))
    fails = Failures()
    try:
        _solve(ctx, fails, case, 1, _want(oracle, lut, case, 1), images=views)
    finally:
        _defaults(ctx)
    fails.done()


def test_exchange_record_in_a_batch(oracle, lut):
    """rtdd_estimate_depth_batch, 3 images, level 0 on the straddling shape of tile 6 at depth 8 as ONE persistent launch over blockIdx.z:
    every image's offsets stay relative to its own planes (the image's offset is folded into the plane pointers) and every image's
    tiles poll flags of their own.  Every level of every image against the oracle's cascade."""
    tile, T, images = 6, 8, 3
    s = next(s for s in xs.shapes(tile, T) if s.tag == "straddle")
    level0 = 2 * T + 3
    iters = level0 << (pyramid_levels(s.rows, s.cols) - 1)
    data = [_bgr(s.rows, s.cols, 900 + b) for b in range(images)]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        c.set_option(rt.OPT_TILE, tile); c.set_option(rt.OPT_TEMPORAL_DEPTH, T)
        levels = c.pyramid_create_batch(s.rows, s.cols, images)
        assert levels >= 2
        for b, (bgr, ann) in enumerate(data):
            c.pyramid_select(b); c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth_batch(iters); c.synchronize()
        info, per_launch = c.pyramid_level_info(0)
        assert (info.kernel, info.tile, info.persistent, info.temporal_depth, per_launch) == (2, tile, 1, T, images), (info.describe(), per_launch)
        assert info.iterations == level0 and tg.persistent_expected(tile, T, s.rows, s.cols, level0, images=images)
        for b, (bgr, ann) in enumerate(data):
            ref = Cascade(oracle, bgr, ann, lut, 1, threads=min(8, oracle.max_threads()))
            ref.estimate(iters)
            _compare(c, b, (ref.depth, ref.depth_u8), f"tile {tile} {s.rows}x{s.cols} x {images}: against the oracle's cascade")
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 0
