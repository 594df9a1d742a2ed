"""Tiny numerators in every sweep (-m gpu): pockets of free pixels enclosed by label-0 strokes whose input depth is set directly to
mixed-sign values of 1e-30, 1e-38, 3e-45 and 1.4e-45, so that the weighted sums of the pocket lie below 2^-100 -- most of them denormal,
with denormal quotients -- from the first sweep on.  That is the branch of the sweep kernels that divides by div_tiny
(csrc/sweep_common.hpp) and falls back to the IEEE divide for a row group with a lane on a midpoint of the denormal grid.  The depth
maps must be the oracle's bit for bit.

  flat    flat gray: every weight is 1 and the divisors are 2 (the image's corner), 3 (its border) and 4 -- the exact ties
  noise   seeded noise: generic divisors
  huge    a Dirichlet depth of 2^99 in the rows of the pockets: lanes of the same row groups whose numerator times 2^64 overflows and
          which must keep the quotient they have

Sizes: 128 x 96 (one 1024-thread tile of three rows per thread) and 240 x 176 (several tiles; the 40 x 7 pocket straddles a tile corner of
tile 4 at depth 8).  Jacobi through tile 4 (the 1080p tile), tile 9 (one row per thread) and tile 14 (the column layout), persistent and
launch per block, 8, 24 and 64 sweeps, both contraction settings; red-black through the one-colour kernel and the register-blocked one."""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from gpu_util import assert_bit_equal_nan_aware, down, up

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (176, 240)]
SWEEPS = (8, 24, 64)
TINY = np.float32([1e-30, -1e-38, 3e-45, -1.4e-45, -1e-30, 1e-38, -3e-45, 1.4e-45])
# (tile, temporal depth, persistent): the 1080p tile as the bench runs it and launch per block; the one-row tile; the column layout
JACOBI = [(4, 8, 1), (4, 8, 0), (9, 4, 1), (9, 4, 0), (14, 4, 0)]
# (kernel option, tile, depth) of RTDD_METHOD_RED_BLACK_GS: one launch per colour; register-blocked, both tile shapes
RED_BLACK = [(1, 0, 0), (0, 1, 4), (0, 2, 5)]


def make(kind, rows, cols):
    rng = np.random.default_rng(7 + rows)
    if kind == "noise":
        gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    elif kind == "huge":
        gray = (128 + rng.integers(0, 4, (rows, cols))).astype(np.uint8)
    else:
        gray = np.full((rows, cols), 128, np.uint8)
    mask = np.full((rows, cols), 32, np.uint8)
    depth = np.full((rows, cols), 255.0, np.float32)
    # a few ordinary strokes, so that the rest of the image is an ordinary solve
    for y, x, lab in ((rows // 2, 5, 200.0), (rows - 9, cols // 2, 64.0)):
        mask[y:y + 3, x:x + 9] = 255; depth[y:y + 3, x:x + 9] = lab
    # the pockets: 12 x 12 in the image's corner (divisors 2 and 3 on its outer pixels), 40 wide and 7 high across x = 112, y = 80 where the image has them
    py, px = (77, 90) if rows > 100 else (60, 70)
    pockets = [(0, 0, 12, 12), (py, px, 7, 40)]
    for y, x, h, w in pockets:
        ya, xa = max(y - 2, 0), max(x - 2, 0)
        mask[ya:y + h + 2, xa:x + w + 2] = 255; depth[ya:y + h + 2, xa:x + w + 2] = 0.0          # the label-0 ring
        mask[y:y + h, x:x + w] = 32
        depth[y:y + h, x:x + w] = TINY[(np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % len(TINY)]
    if kind == "huge":
        for y, x, h, w in pockets:           # in the pocket's rows, a few lanes away from its ring
            xa = x + w + 6
            mask[y + 1:y + 4, xa:xa + 3] = 255; depth[y + 1:y + 4, xa:xa + 3] = np.float32(2.0 ** 99)
    return {"gray": gray, "mask": mask, "depth": depth, "pockets": pockets}


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


def _tiny_sums_met(oracle, lut, p, contract, sweeps):
    """How many pocket pixels still hold a non-zero value below 2^-100 after `sweeps` sweeps: the branch is met to the end."""
    x = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], sweeps, 0, 0, lut, contract)
    n = 0
    for y, xx, h, w in p["pockets"]:
        v = np.abs(x[y:y + h, xx:xx + w])
        n += int(((v > 0) & (v < 2.0 ** -100)).sum())
    return n


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("kind", ["flat", "noise", "huge"])
def test_jacobi_and_red_black_match_the_oracle(ctx, oracle, lut, kind, shape):
    rows, cols = shape
    p = make(kind, rows, cols)
    m, g = up(p["mask"]), up(p["gray"])
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    msgs = []

    def check(got, want, what):
        try:
            assert_bit_equal_nan_aware(got, want, what)
        except AssertionError as e:
            msgs.append(str(e))
    try:
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            assert _tiny_sums_met(oracle, lut, p, contract, 8) > 0, "the pockets no longer hold tiny values: the image does not test what it should"
            for n in SWEEPS:
                want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], n, 0, 0, lut, contract)
                for tile, depth, persistent in JACOBI:
                    ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, tile)
                    ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, persistent)
                    d = up(p["depth"])
                    ctx.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, n, 1e-5, 0)
                    ctx.synchronize()
                    info = ctx.last_solve_info()
                    assert info.kernel == 2, info.describe()
                    check(down(d), want, f"jacobi {kind} {cols}x{rows} contract {contract} x{n} tile {tile} depth {depth} persistent {persistent} [{info.describe()}]")
                x = p["depth"].copy()
                for _ in range(n):
                    oracle.rbgs_sweep(x, idx, p["mask"], lut, contract, 1.0)
                for kernel, tile, depth in RED_BLACK:
                    ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel); ctx.set_option(rt.OPT_TILE, tile)
                    ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, 1)
                    d = up(p["depth"])
                    its, _ = ctx.solve_ex(d, m, g, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=n, tolerance=0.0, relaxation=1.0)
                    ctx.synchronize()
                    info = ctx.last_solve_info()
                    assert its == n and info.kernel == (3 if kernel == 1 else 4), info.describe()
                    check(down(d), x, f"red-black {kind} {cols}x{rows} contract {contract} x{n} [{info.describe()}]")
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1); ctx.set_option(rt.OPT_PERSISTENT, 1)
        for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH):
            ctx.set_option(k, 0)
    assert not msgs, f"{len(msgs)} mismatches:\n" + "\n".join(msgs[:12])
