"""The register-blocked Jacobi sweeps (k_sweep_blocked, k_sweep_col) on shapes derived from each tile's OWN geometry (-m gpu).

tests/tile_geometry.py restates the host's geometry from the tile table and places every shape relative to the centre width and
height, TW x TH, of the (tile, depth) under test: last tile rows / columns of 1 .. halo-1 pixels (alone and together at the corner),
the two widths and heights on either side of the wave-uniform `tile_inside` fast path of the middle tile, one tile row by several
columns and the reverse, tile counts that are and are not a multiple of the 8 XCDs.  tests/test_tile_geometry_cpu.py shows that every
class is there for every (tile, depth) used here.  Every solve must run the path the helper predicts (rtdd_last_solve_info: kernel,
tile, persistence, sweeps of the last block, launches) and give the oracle's bits; no tolerance anywhere."""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import tile_geometry as tg
from cascade_ref import Cascade, pyramid_levels
from gpu_util import bits, down, up
from realtimedepthdiffusion_amd.synth import make_problem
from test_gpu_batch import _compare
from test_gpu_cascade import _bgr

pytestmark = pytest.mark.gpu

K = rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH


@pytest.fixture(scope="module")
def _ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


def _defaults(c):
    c.set_option(rt.OPT_FP_CONTRACT, 1); c.set_option(rt.OPT_PERSISTENT, 1)
    for k in K:
        c.set_option(k, 0)


@pytest.fixture
def ctx(_ctx):
    """The shared context with every option at its default."""
    _defaults(_ctx)
    return _ctx


class Failures:
    """Every failing case of a test is reported, not only the first: a geometry bug then shows its pattern."""

    def __init__(self):
        self.msgs, self.cases = [], 0

    def expect(self, ok, what):
        if not ok:
            self.msgs.append(what)

    def check(self, got, want, what):
        bad = bits(got) != bits(want)
        if bad.any():
            ys, xs = np.nonzero(bad)
            self.msgs.append(f"{what}: {int(bad.sum())} of {got.size} values differ, rows {ys.min()}..{ys.max()}, columns {xs.min()}..{xs.max()}")

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} failures in {self.cases} cases:\n" + "\n".join(self.msgs[:40])


_problems = {}


def _problem(rows, cols):
    """As test_randomised_shapes_and_options builds them: at least one Dirichlet pixel, free pixels uniform in [0, 255], fixed seed."""
    if (rows, cols) not in _problems:
        p = make_problem(rows, cols, seed=5000 + 7 * rows + cols)
        if (p["mask"] == 255).sum() == 0:
            p["mask"][rows // 2, cols // 2] = 255; p["depth"][rows // 2, cols // 2] = 128
        free = p["mask"] != 255
        p["depth"][free] = np.random.default_rng(rows * 1000 + cols).uniform(0, 255, int(free.sum())).astype(np.float32)
        _problems[(rows, cols)] = p
    return _problems[(rows, cols)]


def _variant(i):
    """(contraction, levels) of case i: OPT_FP_CONTRACT alternates 1, 0; (level, levels) alternates (0, 1), the un-gated edge-weight
    rule, and (0, 2), the gated one -- at another period, so that all four combinations meet every kind of sweep count."""
    return 1 - i % 2, 1 + (i // 3) % 2


def _run(ctx, oracle, lut, fails, i, tile, asked, s, n, persistent, reps):
    p = _problem(s.rows, s.cols)
    contract, levels = _variant(i)
    T = tg.geometry(tile, asked).T
    want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], n, 0, levels - 1, lut, contract, threads=min(8, oracle.max_threads()))
    ctx.GPUAllocateDeviceMemory(s.rows, s.cols, levels)
    ctx.set_option(rt.OPT_FP_CONTRACT, contract); ctx.set_option(rt.OPT_PERSISTENT, persistent)
    ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, tile); ctx.set_option(rt.OPT_TEMPORAL_DEPTH, asked)
    m, g = up(p["mask"]), up(p["gray"])
    what = (f"tile {tile} depth {asked}" + (f" (clamped to {T})" if T != asked else "") + f" {s.rows}x{s.cols} [{s.tag}; {tg.grid(tile, asked, s.rows, s.cols)} tiles] "
            f"x{n} contract {contract} levels {levels}")
    path = (2, tile, 1 if persistent else 0, tg.last_block_expected(tile, asked, s.rows, s.cols, n, persistent), tg.launches_expected(tile, asked, s.rows, s.cols, n, persistent))
    for rep in range(reps):                  # (the hand-off flags are epoch based and never reset: a second run meets what the first left)
        d = up(p["depth"])
        ctx.GPUMatrixFreeSolver(d, m, g, s.rows, s.cols, 0.4, n, 0.0, 0)
        ctx.synchronize()
        info = ctx.last_solve_info()
        got_path = (info.kernel, info.tile, info.persistent, info.temporal_depth, info.launches)
        fails.expect(got_path == path and info.iterations == n, f"{what} rep {rep}: ran (kernel, tile, persistent, last block, launches) = {got_path}, expected {path} [{info.describe()}]")
        fails.check(down(d), want, f"{what} rep {rep}")
    fails.cases += 1


@pytest.mark.parametrize("tile", tg.ALL_TILES)
def test_launch_per_block_on_the_tiles_own_edges(ctx, oracle, lut, tile):
    """One launch per block of sweeps (OPT_PERSISTENT = 0), tiles 1-13 in the row layout and 14-16 in the column layout, at depths 1,
    5, 8, the deepest the host's clamp leaves alone and 28 (which the helper must predict the clamp of), sweep counts of T - 1, T,
    T + 1 and 2*T + 3 in turn: a short only block, exactly one, a one-sweep tail (its own, shallower geometry), three launches."""
    fails = Failures()
    try:
        for i, (asked, s, n) in enumerate(tg.launch_per_block_cases(tile)):
            _run(ctx, oracle, lut, fails, i, tile, asked, s, n, 0, 1)
    finally:
        _defaults(ctx)
    fails.expect(ctx.get_option(rt.OPT_TIMEOUT_HEALS) == 0, "a launch reported a time-out and was healed")
    fails.done()


@pytest.mark.parametrize("tile", tg.ROW_TILES)
def test_persistent_on_the_tiles_own_edges(ctx, oracle, lut, tile):
    """One launch, halo strips traded every T sweeps (OPT_PERSISTENT = 1) at every depth of 2, 4, 8, 12, 16, 20 whose halo fits the
    neighbours' centres; sweep counts of T + 1, 2*T, 2*T + 3, 3*T and 4*T + 1 in turn: 2, 2, 3, 3 and 5 blocks -- the result in either
    plane pair -- with tails of 1 and 3 sweeps.  Every case must run persistently, twice back to back, and no launch may time out:
    at most a few dozen workgroups are resident at once on any GPU, so a heal here is a finding and not something to cover up."""
    fails = Failures()
    try:
        for i, (T, s, n) in enumerate(tg.persistent_cases(tile)):
            _run(ctx, oracle, lut, fails, i, tile, T, s, n, 1, 2)
    finally:
        _defaults(ctx)
    fails.expect(ctx.get_option(rt.OPT_TIMEOUT_HEALS) == 0, f"{ctx.get_option(rt.OPT_TIMEOUT_HEALS)} persistent launches timed out and were healed")
    fails.done()


def _options(c, tile):
    c.set_option(rt.OPT_TILE, tile); c.set_option(rt.OPT_TEMPORAL_DEPTH, tg.BATCH_DEPTH)


def _single_image(rows, cols, bgr, ann, iters, tile):
    """[level] depth images and the u8 map of ONE image on a single-image pyramid under the batch's options."""
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        _options(c, tile)
        levels = c.pyramid_create(rows, cols)
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.estimate_depth(iters); c.synchronize()
        info, _ = c.pyramid_level_info(0)
        assert (info.kernel, info.tile, info.persistent) == (2, tile, 1), info.describe()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 0
        return [c.pyramid_download(rt.IMG_DEPTH, l) for l in range(levels)], c.pyramid_download(rt.IMG_DEPTH_U8)


@pytest.mark.parametrize("tile", tg.BATCH_TILES)
def test_a_batch_on_the_tiles_own_edges(oracle, lut, tile):
    """rtdd_estimate_depth_batch with tile and depth fixed runs a level of all images as ONE persistent launch over blockIdx.z, every
    image's tiles with hand-off flags of their own: a shape whose last tile row and column are both ragged and the 4 x 4 shape with
    its one-pixel corner tile, 3 images, every level of every image against a single-image pyramid and against the oracle's cascade."""
    T, images = tg.BATCH_DEPTH, tg.BATCH_IMAGES
    for k, s in enumerate(tg.batch_shapes(tile)):
        rows, cols = s.rows, s.cols
        # level 0 runs maxIterations / 2^(levels - 1) sweeps (src/main.cpp:263): 2*T + 3 and 4*T + 1 there, 3 and 5 blocks, tails of 3 and 1
        level0 = (2 * T + 3, 4 * T + 1)[k]
        iters = level0 << (pyramid_levels(rows, cols) - 1)
        data = [_bgr(rows, cols, 600 + 10 * tile + b) for b in range(images)]
        want = [_single_image(rows, cols, bgr, ann, iters, tile) for bgr, ann in data]
        with rt.Context(0) as c:
            c.GPULoadWeights(0.4)
            _options(c, tile)
            levels = c.pyramid_create_batch(rows, cols, images)
            assert levels >= 2
            for b, (bgr, ann) in enumerate(data):
                c.pyramid_select(b); c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
            c.estimate_depth_batch(iters); c.synchronize()
            info, per_launch = c.pyramid_level_info(0)
            assert (info.kernel, info.tile, info.persistent, info.temporal_depth, per_launch) == (2, tile, 1, T, images), (info.describe(), per_launch)
            assert info.iterations == level0 and tg.persistent_expected(tile, T, rows, cols, level0, images=images)
            for b, (bgr, ann) in enumerate(data):
                _compare(c, b, want[b], f"tile {tile} {rows}x{cols} [{s.tag}] x {images}: against the single-image pyramid")
                ref = Cascade(oracle, bgr, ann, lut, 1, threads=min(8, oracle.max_threads()))
                ref.estimate(iters)
                _compare(c, b, (ref.depth, ref.depth_u8), f"tile {tile} {rows}x{cols} [{s.tag}] x {images}: against the oracle's cascade")
            assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 0
