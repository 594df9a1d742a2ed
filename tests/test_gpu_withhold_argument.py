"""RTDD_OPT_DEBUG_WITHHOLD_TILE reaches a persistent kernel as an ARGUMENT of its launch (csrc/persist_sync.hpp exchange_wait_at), not
as a control word the kernel reads back at every exchange: a launch sees the option's value at the time it was enqueued, whatever the
host sets while it is still queued or running.  (-m gpu)

The sequence, with NO synchronisation in between: queue a solve; set the option to tile 2; queue a second solve; set it to 0; queue a
third.  The first solve must come out untouched by the setting made behind it (the oracle's bits, before any heal); the second must time
out (its buffer still holds its INPUT before the heal) and heal; behind the library's synchronisation all three equal the oracle bit
for bit, with exactly one heal.  A 2 ms poll limit keeps the time-out short.

Shapes: two tiles in each direction of the 1080p tile (tile 4 at depth 8; tests/tile_geometry.py), as tests/test_gpu_tiny_midpoints.py
builds them, two blocks of sweeps.  The red-black kernel goes persistent only from half the chip's compute units up
(csrc/rbgs_blocked.hip launch_rbgs_blocked: a smaller grid is launch-bound), so ITS case is the smallest grid that does: 16 x 8 of its
128 x 64 tile at depth 4.  One case through a batch of two images (the tile of that number is withheld in each image), one with a tile
number beyond the grid, where nothing may happen."""
import numpy as np
import pytest
import torch

import realtimedepthdiffusion_amd as rt
import tile_geometry as tg
from cascade_ref import Cascade
from gpu_util import assert_bit_equal, down, up
from realtimedepthdiffusion_amd.synth import make_problem
from test_gpu_cascade import _bgr

pytestmark = pytest.mark.gpu

TILE, DEPTH = 4, 8               # k_sweep_blocked<32, 1024, 3, ., true>: what a 1080p solve runs
SWEEPS = 2 * DEPTH               # two blocks, one exchange
POLL_LIMIT_US = 2000


def two_by_two(tile, depth):
    g = tg.geometry(tile, depth)
    rows, cols = g.TH + g.hy + 9, g.TW + g.hx + 9
    assert tg.grid(tile, depth, rows, cols) == (2, 2) and tg.persistent_expected(tile, depth, rows, cols, SWEEPS)
    return rows, cols


@pytest.fixture(scope="module")
def jacobi(oracle, lut):
    rows, cols = two_by_two(TILE, DEPTH)
    p = make_problem(rows, cols, seed=77)
    p["want"] = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], SWEEPS, 0, 0, lut, 1)
    return p


def _context(rows, cols, tile, depth):
    c = rt.Context(0)
    c.GPUAllocateDeviceMemory(rows, cols, 1); c.GPULoadWeights(0.4)
    c.set_option(rt.OPT_TILE, tile); c.set_option(rt.OPT_TEMPORAL_DEPTH, depth); c.set_option(rt.OPT_PERSISTENT, 1)
    c.set_option(rt.OPT_DEBUG_POLL_LIMIT_US, POLL_LIMIT_US)
    return c


def _three_solves(c, p, want, queue, what):
    """queue(d) enqueues one solve on depth buffer d; the buffers are uploaded first, so that nothing synchronises inside the sequence."""
    d = [up(p["depth"]) for _ in range(3)]
    torch.cuda.synchronize()
    queue(d[0])
    c.set_option(rt.OPT_DEBUG_WITHHOLD_TILE, 2)
    queue(d[1])
    c.set_option(rt.OPT_DEBUG_WITHHOLD_TILE, 0)
    queue(d[2])
    torch.cuda.synchronize()                                 # (not a library call: nobody has looked at the status word yet)
    assert_bit_equal(down(d[0]), want, f"{what}: the solve queued BEFORE the option was set")
    assert_bit_equal(down(d[1]), p["depth"], f"{what}: the solve queued with tile 2 withheld must have timed out and kept its input")
    c.synchronize()                                          # heals
    assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
    for i in range(3):
        assert_bit_equal(down(d[i]), want, f"{what}: solve {i + 1} of 3 behind the heal")


def test_a_queued_jacobi_launch_keeps_the_value_it_was_enqueued_with(jacobi):
    p = jacobi
    rows, cols = p["gray"].shape
    m, g = up(p["mask"]), up(p["gray"])
    with _context(rows, cols, TILE, DEPTH) as c:
        c.set_option(rt.OPT_SWEEP_KERNEL, 2)
        warm = up(p["depth"])
        c.GPUMatrixFreeSolver(warm, m, g, rows, cols, 0.4, SWEEPS, 0.0, 0); c.synchronize()
        info = c.last_solve_info()
        assert info.kernel == 2 and info.tile == TILE and info.persistent == 1, info.describe()
        _three_solves(c, p, p["want"], lambda d: c.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, SWEEPS, 0.0, 0), f"tile {TILE} {cols}x{rows}")


def test_a_tile_number_beyond_the_grid_withholds_nothing(jacobi):
    p = jacobi
    rows, cols = p["gray"].shape
    m, g = up(p["mask"]), up(p["gray"])
    with _context(rows, cols, TILE, DEPTH) as c:
        c.set_option(rt.OPT_SWEEP_KERNEL, 2)
        for number in (4, 5, 1023):                          # the grid's tiles are 0 .. 3; the option is the number + 1
            c.set_option(rt.OPT_DEBUG_WITHHOLD_TILE, number + 1)
            d = up(p["depth"])
            c.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, SWEEPS, 0.0, 0); c.synchronize()
            info = c.last_solve_info()
            assert info.persistent == 1 and c.get_option(rt.OPT_TIMEOUT_HEALS) == 0, info.describe()
            assert_bit_equal(down(d), p["want"], f"tile number {number} of a 2 x 2 grid withheld")


def test_a_queued_red_black_launch_keeps_the_value_it_was_enqueued_with(oracle, lut):
    tile, depth, n = 1, 4, 8                                 # 128 x 64 tiles, halo 8: centres of 112 x 48
    rows, cols = 8 * 48 - 3, 16 * 112 - 5                    # 16 x 8 = 128 tiles: half of the 256 compute units, the least that runs persistently
    p = make_problem(rows, cols, seed=78)
    m, g = up(p["mask"]), up(p["gray"])
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    want = p["depth"].copy()
    for _ in range(n):
        oracle.rbgs_sweep(want, idx, p["mask"], lut, 1, 1.0)

    with _context(rows, cols, tile, depth) as c:
        def queue(d):
            c.solve_ex(d, m, g, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=n, tolerance=0.0, relaxation=1.0)
        warm = up(p["depth"])
        queue(warm); c.synchronize()
        info = c.last_solve_info()
        assert info.kernel == 4 and info.persistent == 1, info.describe()
        _three_solves(c, p, want, queue, f"red-black {cols}x{rows}")


def test_a_batch_withholds_the_tile_of_that_number_in_every_image(oracle, lut):
    rows, cols = two_by_two(TILE, DEPTH)
    images = 2
    data = [_bgr(rows, cols, 900 + b) for b in range(images)]
    refs = [Cascade(oracle, bgr, ann, lut, 1) for bgr, ann in data]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        levels = c.pyramid_create_batch(rows, cols, images)
        for b, (bgr, ann) in enumerate(data):
            c.pyramid_select(b); c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        c.set_option(rt.OPT_TILE, TILE); c.set_option(rt.OPT_TEMPORAL_DEPTH, DEPTH); c.set_option(rt.OPT_DEBUG_POLL_LIMIT_US, POLL_LIMIT_US)
        iters = SWEEPS << (levels - 1)                       # level l runs iters / 2^(levels - 1 - l) sweeps (src/main.cpp:263): two blocks at level 0

        def check(what):
            for b in range(images):
                c.pyramid_select(b)
                for l in range(levels):
                    assert_bit_equal(c.pyramid_download(rt.IMG_DEPTH, l), refs[b].depth[l], f"{what}: image {b}, level {l}")
                assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), refs[b].depth_u8), f"{what}: image {b}, u8 map"
        c.estimate_depth_batch(iters); c.synchronize()
        info, per_launch = c.pyramid_level_info(0)
        assert info.tile == TILE and info.persistent == 1 and per_launch == images, info.describe()      # one launch, 2 x 4 tiles
        for r in refs:
            r.estimate(iters)
        check("cold, nothing withheld")
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 0
        c.set_option(rt.OPT_DEBUG_WITHHOLD_TILE, 2)          # tile 1 of image 0 and tile 1 of image 1
        c.estimate_depth_batch(iters); c.synchronize()
        assert c.get_option(rt.OPT_TIMEOUT_HEALS) == 1
        for r in refs:
            r.estimate(iters)
        check("warm start, tile 1 of every image withheld, healed")
