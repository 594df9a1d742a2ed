"""Stationary denormal pixels on and around the midpoints of the denormal grid (-m gpu): the case of a converged photograph, which the
decaying pockets of tests/test_gpu_tiny_numerators.py rarely hold.

The pocket is a checkerboard enclosed by a label-0 ring (built as that test's `make` builds its pockets): its even pixels are Dirichlet
with depths of 2^20 .. 2^23 units of 2^-149, its odd pixels are free, over seeded low-contrast noise -- generic weights, none of them denormal.  A free pixel's four
neighbours never change, so its numerator is the same tiny number at every sweep and its quotient is denormal; among a few hundred of
them some 24-bit quotients land exactly on a midpoint of the 2^-149 grid, the lanes the two-rounding divide had to hand to the IEEE
divide at every sweep.  div_tiny (csrc/sweep_common.hpp) now rounds once: every result must be the oracle's bit for bit.

Shapes come from each tile's own geometry (tests/tile_geometry.py): two tiles in each direction, the pocket across the tile corner.
k_sweep_blocked on tile 3, tile 4 and the one-row tile 9, launch per block and persistent; k_sweep_col (tile 14); k_rbgs_blocked; both
settings of RTDD_OPT_FP_CONTRACT.  The test first asserts on the CPU that the pocket's numerators ARE tiny and that midpoints ARE met."""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import tile_geometry as tg
from gpu_util import assert_bit_equal_nan_aware, down, up

pytestmark = pytest.mark.gpu

# (tile, temporal depth, persistent) of the Jacobi kernels; (tile, depth) of the register-blocked red-black kernel
JACOBI = [(3, 4, 0), (3, 4, 1), (4, 8, 0), (4, 8, 1), (9, 4, 0), (9, 4, 1), (14, 4, 0)]
RED_BLACK = [(1, 4), (2, 5)]
SWEEPS = (9, 24)                 # more than one block of every depth above, an odd and an even count


def make(tile, depth):
    g = tg.geometry(tile, depth)
    rows, cols = g.TH + g.hy + 9, g.TW + g.hx + 9                     # 2 x 2 tiles, the second row and column a little more than a halo
    assert tg.grid(tile, depth, rows, cols) == (2, 2)
    rng = np.random.default_rng(11 + tile)
    gray = (120 + rng.integers(0, 12, (rows, cols))).astype(np.uint8)                # weights between e^0 and e^-4.4: generic divisors, no denormal weight
    mask = np.full((rows, cols), 32, np.uint8)
    depth_img = np.full((rows, cols), 255.0, np.float32)
    mask[3:6, 4:13] = 255; depth_img[3:6, 4:13] = 64.0                # an ordinary stroke: the rest of the image is an ordinary solve
    h, w = 10, 24
    y, x = g.TH - h // 2, g.TW - w // 2                               # across the corner where the four tiles meet
    mask[y - 2:y + h + 2, x - 2:x + w + 2] = 255; depth_img[y - 2:y + h + 2, x - 2:x + w + 2] = 0.0      # the label-0 ring
    yy, xx = np.mgrid[0:h, 0:w]
    units = rng.integers(1 << 20, 1 << 23, (h, w)).astype(np.uint32)  # the top binades of the denormals: a 24-bit quotient has 1 - 3 bits below the grid
    vals = units.view(np.float32).copy()                              # units of 2^-149, as bit patterns
    vals[(yy * 5 + xx) % 3 == 0] *= -1
    even = (yy + xx) % 2 == 0
    m = mask[y:y + h, x:x + w]; d = depth_img[y:y + h, x:x + w]
    m[even] = 255; d[even] = vals[even]
    m[~even] = 32; d[~even] = np.float32(1e-40)
    return {"gray": gray, "mask": mask, "depth": depth_img, "pocket": (y, x, h, w), "free": ~even}


def census(oracle, lut, p, contract):
    """(free pocket pixels with a tiny numerator, those of them whose 24-bit scaled quotient is a midpoint of the 2^-149 grid) after a sweep."""
    x = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], 1, 0, 0, lut, contract).astype(np.float64)
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    w = [lut[idx[..., 0] // 1000], lut[idx[..., 0] % 1000], lut[idx[..., 1] // 1000], lut[idx[..., 1] % 1000]]
    cnt = np.float32(0)
    for k in range(4):
        cnt = (cnt + w[k]).astype(np.float32)
    cnt = np.where(cnt == 0, np.float32(1), cnt).astype(np.float64)
    z = np.zeros_like(x)
    nb = [z.copy(), z.copy(), z.copy(), z.copy()]
    nb[0][:, 1:] = x[:, :-1]; nb[1][:, :-1] = x[:, 1:]; nb[2][1:] = x[:-1]; nb[3][:-1] = x[1:]
    sm = np.zeros(x.shape, np.float32)
    for k in range(4):
        sm = (w[k].astype(np.float64) * nb[k] + sm.astype(np.float64)).astype(np.float32)
    y, xx, h, ww = p["pocket"]
    sel = np.zeros(x.shape, bool); sel[y:y + h, xx:xx + ww] = p["free"]
    tiny = sel & (np.abs(sm) < np.float32(2.0 ** -100)) & (sm != 0)
    with np.errstate(all="ignore"):
        Q = np.where(tiny, sm.astype(np.float64) * 2.0 ** 64 / cnt, 0.0).astype(np.float32)
        q = (Q * np.float32(2.0 ** -64)).astype(np.float32)
    mid = tiny & (np.abs(Q.astype(np.float64) - q.astype(np.float64) * 2.0 ** 64) == 2.0 ** -86)
    return int(tiny.sum()), int(mid.sum())


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


def _reset(ctx):
    ctx.set_option(rt.OPT_FP_CONTRACT, 1); ctx.set_option(rt.OPT_PERSISTENT, 1)
    for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH):
        ctx.set_option(k, 0)


@pytest.mark.parametrize("tile,depth,persistent", JACOBI)
def test_jacobi_on_stationary_midpoints(ctx, oracle, lut, tile, depth, persistent):
    p = make(tile, depth)
    rows, cols = p["gray"].shape
    m, g = up(p["mask"]), up(p["gray"])
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    msgs = []
    try:
        for contract in (1, 0):
            tiny, mid = census(oracle, lut, p, contract)
            assert tiny >= 100 and mid >= 1, f"{tiny} tiny numerators, {mid} on a midpoint: the pocket does not test what it should"
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            for n in SWEEPS:
                want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], n, 0, 0, lut, contract)
                ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, tile)
                ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, persistent)
                d = up(p["depth"])
                ctx.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, n, 1e-5, 0)
                ctx.synchronize()
                info = ctx.last_solve_info()
                assert info.kernel == 2 and info.tile == tile, info.describe()
                try:
                    assert_bit_equal_nan_aware(down(d), want, f"tile {tile} depth {depth} persistent {persistent} contract {contract} x{n} {cols}x{rows} [{info.describe()}]")
                except AssertionError as e:
                    msgs.append(str(e))
    finally:
        _reset(ctx)
    assert not msgs, f"{len(msgs)} mismatches:\n" + "\n".join(msgs)


@pytest.mark.parametrize("tile,depth", RED_BLACK)
def test_red_black_on_stationary_midpoints(ctx, oracle, lut, tile, depth):
    p = make(4, 8)
    rows, cols = p["gray"].shape
    m, g = up(p["mask"]), up(p["gray"])
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    msgs = []
    try:
        for contract in (1, 0):
            tiny, mid = census(oracle, lut, p, contract)
            assert tiny >= 100 and mid >= 1, f"{tiny} tiny numerators, {mid} on a midpoint"
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            x = p["depth"].copy()
            done = 0
            for n in SWEEPS:
                for _ in range(n - done):
                    oracle.rbgs_sweep(x, idx, p["mask"], lut, contract, 1.0)
                done = n
                ctx.set_option(rt.OPT_SWEEP_KERNEL, 0); ctx.set_option(rt.OPT_TILE, tile)
                ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, 1)
                d = up(p["depth"])
                its, _ = ctx.solve_ex(d, m, g, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=n, tolerance=0.0, relaxation=1.0)
                ctx.synchronize()
                info = ctx.last_solve_info()
                assert its == n and info.kernel == 4, info.describe()
                try:
                    assert_bit_equal_nan_aware(down(d), x, f"red-black tile {tile} depth {depth} contract {contract} x{n} [{info.describe()}]")
                except AssertionError as e:
                    msgs.append(str(e))
    finally:
        _reset(ctx)
    assert not msgs, f"{len(msgs)} mismatches:\n" + "\n".join(msgs)
