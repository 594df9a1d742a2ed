"""Scaled mode of the persistent Jacobi sweep (-m gpu; csrc/sweep_blocked.hip, csrc/sweep_common.hpp div_scaled).

A wave of a persistent launch that has met numerators below 2^-100 during a block of sweeps divides EVERY pixel by div_scaled from the
next halo exchange on, to the end of the launch -- unless the solve's input holds a depth of 2^32 or more (persist_sync.hpp kSyncLarge).
The depth maps must be the oracle's bit for bit whether the mode is entered or not, and every case checks that it was (or was not)
through the count of waves that entered it (rtdd_scaled_mode_waves): no case can pass with the mode never used.

Images as tests/test_gpu_tiny_numerators.py builds them: an ordinary solve with two pockets of free pixels enclosed by label-0 strokes,
12 x 12 in the image's corner and 40 x 7 in its middle, at 128 x 96 (one tile of the 1080p kind) and 240 x 176 (3 x 3 tiles at depth 8;
the 40 x 7 pocket lies across the corner (112, 80) of tile 4's centres).  What the pockets start with, and what lies beside them:

  tiny        the TINY pattern (1e-30 .. 1.4e-45, mixed signs): tiny sums from the first sweep, the mode is entered behind block 1
  tiny_noise  the same on seeded noise: generic weights and divisors
  decaying    1e-28 everywhere in the pockets: ordinary numerators at first, which decay below 2^-100 during the solve -- the test finds
              the oracle's first tiny numerator from the oracle's own iterates and requires it in sweeps 9 .. 48, so the switch happens
              at a block boundary inside the solve.  At 240 x 176 the pocket's part right of x = 112 starts at 1e-26 and gets there some
              blocks later than the part left of it: neighbouring tiles switch at different blocks (asserted on the oracle's iterates)
  beside_2p31 TINY pockets and a Dirichlet depth of 2^31 in the pockets' rows: large, but below the bound -- the mode is entered
  beside_2p99 ... of 2^99 (the `huge` kind of tests/test_gpu_tiny_numerators.py): the mode is NOT entered, the count stays

Every image through persistent tile 4 at depth 8 and persistent tile 9 at depth 4, both contraction settings, 64 sweeps; then the same
through one launch per block of sweeps, where the count stays as well.  (128 x 96 is a single tile of tile 4, which the library runs as
one launch of 64 sweeps whatever is asked: the count stays there too.  Tile 4's persistent cases are the 240 x 176 ones.)"""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
from gpu_util import assert_bit_equal_nan_aware, down, up

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (176, 240)]
SWEEPS = 64
TINY = np.float32([1e-30, -1e-38, 3e-45, -1.4e-45, -1e-30, 1e-38, -3e-45, 1.4e-45])
CONFIGS = [(4, 8), (9, 4)]                     # (tile, temporal depth)
KINDS = ["tiny", "tiny_noise", "decaying", "beside_2p31", "beside_2p99"]
TW4, TH4 = 4 * 32 - 2 * 8, 1024 // 32 * 3 - 2 * 8          # tile 4's centre at depth 8: 112 x 80 of its 128 x 96


def make(kind, rows, cols):
    rng = np.random.default_rng(7 + rows)
    if kind == "tiny_noise":
        gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    elif kind.startswith("beside"):
        gray = (128 + rng.integers(0, 4, (rows, cols))).astype(np.uint8)
    else:
        gray = np.full((rows, cols), 128, np.uint8)          # flat: every weight is 1
    mask = np.full((rows, cols), 32, np.uint8)
    depth = np.full((rows, cols), 255.0, np.float32)
    for y, x, lab in ((rows // 2, 5, 200.0), (rows - 9, cols // 2, 64.0)):
        mask[y:y + 3, x:x + 9] = 255; depth[y:y + 3, x:x + 9] = lab
    py, px = (77, 90) if rows > 100 else (60, 70)
    pockets = [(0, 0, 12, 12), (py, px, 7, 40)]
    for y, x, h, w in pockets:
        ya, xa = max(y - 2, 0), max(x - 2, 0)
        mask[ya:y + h + 2, xa:x + w + 2] = 255; depth[ya:y + h + 2, xa:x + w + 2] = 0.0          # the label-0 ring
        mask[y:y + h, x:x + w] = 32
        if kind == "decaying":
            depth[y:y + h, x:x + w] = np.float32(1e-28)
            if rows > 100 and x > 0:
                depth[y:y + h, TW4:x + w] = np.float32(1e-26)
        else:
            depth[y:y + h, x:x + w] = TINY[(np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % len(TINY)]
    if kind.startswith("beside"):
        big = np.float32(2.0 ** 31 if kind == "beside_2p31" else 2.0 ** 99)
        for y, x, h, w in pockets:               # in the pocket's rows, a few lanes away from its ring
            xa = x + w + 6
            mask[y + 1:y + 4, xa:xa + 3] = 255; depth[y + 1:y + 4, xa:xa + 3] = big
    return {"gray": gray, "mask": mask, "depth": depth, "pockets": pockets}


def tiny_numerators(x, mask):
    """Where a sweep over the iterate x of a FLAT image (every weight 1) forms a numerator with 0 < |sum| < 2^-100: the sum of the four
    neighbours in the kernels' order (left, right, up, down; absent neighbours 0), free pixels only."""
    p = np.pad(x, 1).astype(np.float32)
    s = np.float32(0) + p[1:-1, :-2]; s = s + p[1:-1, 2:]; s = s + p[:-2, 1:-1]; s = s + p[2:, 1:-1]
    s = np.abs(s)
    return (mask != 255) & (s > 0) & (s < np.float32(2.0 ** -100))


def first_tiny_sweep(oracle, lut, p, contract, inside=None):
    """The first sweep of the oracle's own solve that meets a tiny numerator (inside the (y0, y1, x0, x1) window, if given); None: never."""
    for k in range(SWEEPS):
        x = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], k, 0, 0, lut, contract) if k else p["depth"]
        hit = tiny_numerators(x, p["mask"])
        if inside is not None:
            y0, y1, x0, x1 = inside
            hit = hit[max(y0, 0):y1, max(x0, 0):x1]
        if hit.any():
            return k
    return None


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


def check_the_input(oracle, lut, kind, p, rows, cols, contract):
    y, x, h, w = p["pockets"][1]
    if rows > 100:          # the pocket lies across a corner of tile 4's centres
        assert x < TW4 < x + w and y < TH4 < y + h
    if kind in ("tiny", "tiny_noise"):
        # mixed rows: a row of the pocket, as far as one thread row of tile 4's first tile column holds it (128 pixels from x = -8 at 240 x 176,
        # the whole row at 128 x 96; tile 9's thread rows are 64 wide and hold all three kinds as well), has 255-valued free pixels, Dirichlet
        # pixels and denormal free pixels: ordinary numerators go through the scaled form in the same wave as the tiny ones
        row, free = p["depth"][y + 2][:120], p["mask"][y + 2][:120] != 255
        assert (free & (row == 255.0)).any() and (~free).any() and (free & (np.abs(row) > 0) & (np.abs(row) < 2.0 ** -126)).any()
    if kind == "decaying":
        first = first_tiny_sweep(oracle, lut, p, contract)
        print(f"decaying {cols}x{rows} contract {contract}: the oracle's first tiny numerator is in sweep {first}")
        assert first is not None and 9 <= first <= 48, first
        if rows > 100:      # tile columns 0 and 1 of tile 4 at depth 8 (extended tiles) meet their first tiny numerator in different blocks
            left = first_tiny_sweep(oracle, lut, p, contract, (0, rows, -8, -8 + 128))
            right = first_tiny_sweep(oracle, lut, p, contract, (0, rows, TW4 - 8, TW4 - 8 + 128))
            print(f"  tile column 0: sweep {left}, tile column 1: sweep {right}")
            assert left is not None and right is not None and left // 8 != right // 8, (left, right)
    else:
        # tiny from the first sweep, and still after 8
        x8 = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], 8, 0, 0, lut, contract)
        for it in (p["depth"], x8):
            v = np.abs(it[y:y + h, x:x + w])
            assert ((v > 0) & (v < 2.0 ** -100)).any()


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("kind", KINDS)
def test_scaled_mode_matches_the_oracle_and_is_entered(ctx, oracle, lut, kind, shape):
    rows, cols = shape
    p = make(kind, rows, cols)
    m, g = up(p["mask"]), up(p["gray"])
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    entered_expected = kind != "beside_2p99"
    msgs = []
    try:
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            check_the_input(oracle, lut, kind, p, rows, cols, contract)
            want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], SWEEPS, 0, 0, lut, contract)
            for persistent in (1, 0):
                for tile, depth in CONFIGS:
                    ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, tile)
                    ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth); ctx.set_option(rt.OPT_PERSISTENT, persistent)
                    before = ctx.scaled_mode_waves()
                    d = up(p["depth"])
                    ctx.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, SWEEPS, 1e-5, 0)
                    ctx.synchronize()
                    entered = ctx.scaled_mode_waves() - before
                    info = ctx.last_solve_info()
                    what = f"{kind} {cols}x{rows} contract {contract} tile {tile} depth {depth} persistent {persistent} [{info.describe()}]"
                    print(f"{what}: {entered} waves entered scaled mode")
                    # (128 x 96 is ONE tile of tile 4: the library runs it as a single launch of all 64 sweeps, no halo and nothing persistent
                    # about it -- there the count must stay, like in a launch per block)
                    one_tile = tile == 4 and rows <= 96
                    ran_persistent = persistent == 1 and not one_tile
                    assert info.kernel == 2 and info.tile == tile and info.persistent == int(ran_persistent), what
                    assert info.temporal_depth == (SWEEPS if one_tile else depth) and (info.launches == 1) == (ran_persistent or one_tile), what
                    if ran_persistent and entered_expected:
                        # (tile 4 at 240 x 176: each of the four tiles that share the pocket's corner holds pocket pixels in its centre)
                        least = 4 if (tile == 4 and rows > 100) else 1
                        if entered < least:
                            msgs.append(f"{what}: {entered} waves entered scaled mode, at least {least} expected")
                    elif entered != 0:
                        msgs.append(f"{what}: {entered} waves entered scaled mode, none expected")
                    try:
                        assert_bit_equal_nan_aware(down(d), want, what)
                    except AssertionError as e:
                        msgs.append(str(e))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1); ctx.set_option(rt.OPT_PERSISTENT, 1)
        for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH):
            ctx.set_option(k, 0)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:12])
