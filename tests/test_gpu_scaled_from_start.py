"""Scaled mode entered at sweep 0, and the four-operation divide behind it (-m gpu; csrc/sweep_blocked.hip kFromStart, csrc/sweep_common.hpp div_scaled4).

In a persistent launch of the from-start tile (tile 4, <32, 1024, 3>: the 1080p tile) every wave that may enter scaled mode enters it behind
the tile setup, converts its divisors and reciprocals to d * 2^64 and y * 2^-64 and divides every pixel of every sweep by div_scaled4 --
ordinary numerators included.  The other persistent tiles enter on demand, at the block boundary behind a block that met tiny sums, and keep
the seven-operation div_scaled.  Either way the depth map must be the oracle's bit for bit, and the count of waves that entered
(rtdd_scaled_mode_waves, one add per WORKGROUP for the waves that entered at the start) says which path ran.

240 x 176 through tile 4 at depth 8 is 3 x 3 tiles of 16 waves -- the smallest shape at which a tile trades halos with eight neighbours --
and through tile 9 at depth 4 a grid of on-demand tiles.  64 sweeps, both contraction settings.

  image         tile 4 (from the start)                               tile 9 (on demand)
  noise         exactly 9 x 16 = 144: every wave, no tiny sum needed  0: nothing asks for the mode
  tiny_noise    144 less the waves that hold a denormal divisor (full-range noise has a few; counted from the image, below)   at least 1
  beside_2p31   144: a Dirichlet depth of 2^31 is below the bound     at least 1
  beside_2p33   0: the solve holds a depth of 2^32 or more            0        (the fast pair runs, div_tiny in the pockets)
  beside_2p99   0                                                     0
  denormal      143: ONE pixel's four weights are the denormal w[255], its divisor is denormal, its wave runs the IEEE variant
  decaying      144                                                   at least 1, and the oracle's first tiny sum lies behind block 0:
                                                                      the mode is entered at a block boundary inside the solve
"""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from gpu_util import assert_bit_equal_nan_aware, down, up
from test_gpu_scaled_mode import TH4, TW4, check_the_input, make

pytestmark = pytest.mark.gpu

ROWS, COLS, SWEEPS = 176, 240, 64
TILES4, WAVES4 = 3 * 3, 1024 // 64
KINDS = ["noise", "tiny_noise", "beside_2p31", "beside_2p33", "beside_2p99", "denormal", "decaying"]
# kind -> (waves that must have entered through tile 4 at depth 8 BEFORE the waves that hold a denormal divisor are taken off, lower bound or exact 0 through tile 9 at depth 4)
EXPECT = {"noise": (TILES4 * WAVES4, 0), "tiny_noise": (TILES4 * WAVES4, 1), "beside_2p31": (TILES4 * WAVES4, 1), "beside_2p33": (0, 0), "beside_2p99": (0, 0),
          "denormal": (TILES4 * WAVES4, None), "decaying": (TILES4 * WAVES4, 1)}


def weights(gray, lut):
    """(left, right, up, down) weight of every pixel, absent neighbours 0."""
    g = gray.astype(np.int32)
    wr = np.zeros(g.shape, np.float32); wd = np.zeros(g.shape, np.float32)
    wr[:, :-1] = lut[np.abs(g[:, 1:] - g[:, :-1])]
    wd[:-1, :] = lut[np.abs(g[1:, :] - g[:-1, :])]
    wl = np.zeros_like(wr); wl[:, 1:] = wr[:, :-1]
    wu = np.zeros_like(wd); wu[1:, :] = wd[:-1, :]
    return wl, wr, wu, wd


def divisors(gray, lut):
    """The divisor of every pixel: the sum of its four weights in the kernels' order (left, right, up, down)."""
    wl, wr, wu, wd = weights(gray, lut)
    c = np.float32(0) + wl; c = c + wr; c = c + wu; c = c + wd
    return c


def ieee_waves_of_tile_4(gray, lut):
    """How many waves of tile 4's grid at depth 8 hold a pixel with a denormal divisor and therefore run the IEEE variant: per tile the
    128 x 96 extended tile from (bx * 112 - 8, by * 80 - 8), a wave two thread rows of three pixel rows each.  The kernel's own divisors:
    the first pixel of an extended row has no left weight and the last no right weight (sweep_tile_setup.inc), pixels outside the image
    have the divisor 1."""
    wl, wr, wu, wd = weights(gray, lut)
    n = 0
    for by in range(3):
        for bx in range(3):
            x0, y0 = bx * TW4 - 8, by * TH4 - 8
            for wave in range(WAVES4):
                ya, yb = max(y0 + 6 * wave, 0), min(y0 + 6 * wave + 6, ROWS)
                xa, xb = max(x0, 0), min(x0 + 128, COLS)
                if ya >= yb:
                    continue
                l, r = wl[ya:yb, xa:xb].copy(), wr[ya:yb, xa:xb].copy()
                if x0 >= 0:
                    l[:, 0] = 0
                if x0 + 128 <= COLS:
                    r[:, -1] = 0
                c = np.float32(0) + l; c = c + r; c = c + wu[ya:yb, xa:xb]; c = c + wd[ya:yb, xa:xb]
                n += bool(((c < np.float32(2.0 ** -126)) & (c != 0)).any())
    return n


def build(kind, lut):
    if kind in ("noise", "denormal"):
        rng = np.random.default_rng(11)
        gray = (100 + rng.integers(0, 64, (ROWS, COLS))).astype(np.uint8)          # differences below 64: every weight is far from the denormals
        mask = np.full((ROWS, COLS), 32, np.uint8)
        depth = rng.uniform(16.0, 255.0, (ROWS, COLS)).astype(np.float32)
        for y, x, lab in ((ROWS // 2, 5, 200.0), (ROWS - 9, COLS // 2, 64.0), (20, 150, 128.0)):
            mask[y:y + 3, x:x + 9] = 255; depth[y:y + 3, x:x + 9] = lab
        if kind == "denormal":
            # (120, 170) lies in the extended tile of the middle tile of tile 4's grid only (x 104 .. 231, y 72 .. 167; the neighbours' end at
            # x = 119 / begin at 216, end at y = 87 / begin at 152): one wave of one workgroup holds it
            y, x = 120, 170
            gray[y, x] = 255
            gray[y, x - 1] = gray[y, x + 1] = gray[y - 1, x] = gray[y + 1, x] = 0
        c = divisors(gray, lut)
        small = (c < np.float32(2.0 ** -126)) & (c > 0)
        assert small.sum() == (1 if kind == "denormal" else 0), small.sum()
        if kind == "denormal":
            assert small[120, 170] and 119 < 170 < 216 and 87 < 120 < 152
        return {"gray": gray, "mask": mask, "depth": depth, "pockets": []}
    if kind == "beside_2p33":
        p = make("beside_2p31", ROWS, COLS)
        big = p["depth"] == np.float32(2.0 ** 31)
        assert big.any()
        p["depth"][big] = np.float32(2.0 ** 33)
        return p
    return make(kind, ROWS, COLS)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_from_start_and_on_demand_match_the_oracle_and_count_their_waves(ctx, oracle, lut, kind):
    p = build(kind, lut)
    m, g = up(p["mask"]), up(p["gray"])
    ctx.GPUAllocateDeviceMemory(ROWS, COLS, 1)
    from_start, on_demand = EXPECT[kind]
    if from_start:          # every wave of the grid but those that hold a denormal divisor (full-range noise has a few: they run the IEEE variant)
        ieee = ieee_waves_of_tile_4(p["gray"], lut)
        print(f"{kind}: {ieee} waves of tile 4's grid hold a denormal divisor")
        assert ieee == (1 if kind == "denormal" else ieee) and (kind != "noise" or ieee == 0) and ieee < 16, ieee
        from_start = TILES4 * WAVES4 - ieee
    msgs = []
    try:
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            if kind in ("tiny_noise", "decaying", "beside_2p31", "beside_2p99"):
                check_the_input(oracle, lut, kind, p, ROWS, COLS, contract)          # (decaying: the first tiny sum lies in sweeps 9 .. 48)
            want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], SWEEPS, 0, 0, lut, contract)
            for tile, depth, expected, exact in ((4, 8, from_start, True), (9, 4, on_demand, on_demand == 0)):
                ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, tile)
                ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, 1)
                before = ctx.scaled_mode_waves()
                d = up(p["depth"])
                ctx.GPUMatrixFreeSolver(d, m, g, ROWS, COLS, 0.4, SWEEPS, 1e-5, 0)
                ctx.synchronize()
                entered = ctx.scaled_mode_waves() - before
                info = ctx.last_solve_info()
                what = f"{kind} {COLS}x{ROWS} contract {contract} tile {tile} depth {depth} [{info.describe()}]"
                print(f"{what}: {entered} waves entered scaled mode")
                assert info.kernel == 2 and info.tile == tile and info.persistent == 1 and info.launches == 1 and info.temporal_depth == depth, what
                if expected is not None and (entered != expected if exact else entered < expected):
                    msgs.append(f"{what}: {entered} waves entered scaled mode, {'exactly' if exact else 'at least'} {expected} expected")
                try:
                    assert_bit_equal_nan_aware(down(d), want, what)
                except AssertionError as e:
                    msgs.append(str(e))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1); ctx.set_option(rt.OPT_PERSISTENT, 1)
        for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH):
            ctx.set_option(k, 0)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:12])
