"""The lean scaled sweep pair of the from-start tile on the GPU (-m gpu; csrc/sweep_tile_sweeps.inc SCALED && kFromStart: the weighted sum
started at its left term without the `0 +`, gamma in one register for the launch, the update's fma as one three-address instruction).

336 x 240 through tile 4 at depth 8 is 3 x 3 tiles whose centres are 112 x 80: the smallest image at which tile 4 runs persistently and a
tile has neighbours on every side.  24 sweeps are three blocks and two exchanges, 17 sweeps end in an odd tail.  Both contraction
settings.  Inputs, all below 2^32 in magnitude so that every wave may enter scaled mode:

  synthetic       the synthetic problem as it is
  out_of_range    wild_depth.out_of_range: free pixels in [-300, 600] with -0.0, -1, 255 and 256 sprinkled in
  tiny_free       every free pixel +-10^e, e in [-33, -27]: products that underflow, sums of either sign around and below 2^-100
  on_dirichlet    -0.0, negative depths and +-1e-30 on labelled pixels only (they survive every sweep), free pixels in range

The depth map must be oracle.solve's bit for bit, and rtdd_scaled_mode_waves must have risen by every wave of the grid that holds no
denormal divisor: the lean pair is then the code that ran."""
import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import wild_depth
from gpu_util import assert_bit_equal_nan_aware, down, up
from realtimedepthdiffusion_amd.synth import make_problem
from test_gpu_scaled_from_start import weights

pytestmark = pytest.mark.gpu

ROWS, COLS = 240, 336
TW4, TH4, HALO = 112, 80, 8                     # tile 4's centre at depth 8, of its 128 x 96 extended tile
WAVES4, WAVE_ROWS = 1024 // 64, 6               # a wave: two thread rows of three pixel rows
KINDS = ["synthetic", "out_of_range", "tiny_free", "on_dirichlet"]
SEED = 2900


def tiny_free(rows, cols, seed):
    p = wild_depth.base_problem(rows, cols, seed); rng = np.random.default_rng(seed)
    free = np.flatnonzero(p["mask"] != 255)
    v = (10.0 ** rng.uniform(-33, -27, free.size)) * rng.choice([-1.0, 1.0], free.size)
    p["depth"].reshape(-1)[free] = v.astype(np.float32)
    return p


def build(kind):
    if kind == "synthetic":
        return make_problem(ROWS, COLS, seed=SEED)
    if kind == "out_of_range":
        return wild_depth.out_of_range(ROWS, COLS, SEED)
    if kind == "tiny_free":
        return tiny_free(ROWS, COLS, SEED)
    return wild_depth._special_on_dirichlet(np.float32([-0.0, -1.0, -300.0, 1e-30, -1e-30, -2.5e-38]), 0.5)(ROWS, COLS, SEED)


def eligible_waves(gray, lut):
    """The waves of tile 4's 3 x 3 grid at depth 8 that hold no denormal divisor (those run the IEEE variant and never enter scaled mode);
    the kernel's own divisors: the first pixel of an extended row has no left weight and the last no right weight."""
    wl, wr, wu, wd = weights(gray, lut)
    n = 0
    for by in range(3):
        for bx in range(3):
            x0, y0 = bx * TW4 - HALO, by * TH4 - HALO
            for wave in range(WAVES4):
                ya, yb = max(y0 + WAVE_ROWS * wave, 0), min(y0 + WAVE_ROWS * (wave + 1), ROWS)
                xa, xb = max(x0, 0), min(x0 + 128, COLS)
                if ya < yb:
                    l, r = wl[ya:yb, xa:xb].copy(), wr[ya:yb, xa:xb].copy()
                    if x0 >= 0:
                        l[:, 0] = 0
                    if x0 + 128 <= COLS:
                        r[:, -1] = 0
                    c = np.float32(0) + l; c = c + r; c = c + wu[ya:yb, xa:xb]; c = c + wd[ya:yb, xa:xb]
                    if ((c < np.float32(2.0 ** -126)) & (c != 0)).any():
                        continue
                n += 1
    return n


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def problems():
    return {kind: build(kind) for kind in KINDS}


def test_the_inputs_are_what_they_claim(problems):
    for kind, p in problems.items():
        assert np.isfinite(p["depth"]).all() and np.abs(p["depth"]).max() < 2.0 ** 32, kind
    free = problems["out_of_range"]["mask"] != 255
    d = problems["out_of_range"]["depth"]
    assert (d[free] < 0).any() and (np.signbit(d[free]) & (d[free] == 0)).any()
    d = problems["tiny_free"]["depth"]; free = problems["tiny_free"]["mask"] != 255
    assert free.any() and (np.abs(d[free]) < 1e-26).all() and (d[free] < 0).any() and (d[free] > 0).any()
    d = problems["on_dirichlet"]["depth"]; lab = problems["on_dirichlet"]["mask"] == 255
    assert (np.signbit(d[lab]) & (d[lab] == 0)).any() and (d[lab] == np.float32(-300.0)).any() and (d[lab] == np.float32(-1e-30)).any()
    assert (d[~lab] >= 0).all()


@pytest.mark.parametrize("sweeps", [24, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_the_lean_pair_matches_the_oracle_and_is_what_ran(ctx, oracle, lut, problems, kind, sweeps):
    p = problems[kind]
    m, g = up(p["mask"]), up(p["gray"])
    ctx.GPUAllocateDeviceMemory(ROWS, COLS, 1)
    expected = eligible_waves(p["gray"], lut)
    assert 9 * WAVES4 - 16 < expected <= 9 * WAVES4, expected
    msgs = []
    try:
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            want = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], sweeps, 0, 0, lut, contract)
            ctx.set_option(rt.OPT_SWEEP_KERNEL, 2); ctx.set_option(rt.OPT_TILE, 4)
            ctx.set_option(rt.OPT_TEMPORAL_DEPTH, 8); ctx.set_option(rt.OPT_PERSISTENT, 1)
            before = ctx.scaled_mode_waves()
            d = up(p["depth"])
            ctx.GPUMatrixFreeSolver(d, m, g, ROWS, COLS, 0.4, sweeps, 1e-5, 0)
            ctx.synchronize()
            entered = ctx.scaled_mode_waves() - before
            info = ctx.last_solve_info()
            what = f"{kind} {COLS}x{ROWS} x {sweeps} contract {contract} [{info.describe()}]"
            print(f"{what}: {entered} waves entered scaled mode, {expected} eligible")
            assert info.kernel == 2 and info.tile == 4 and info.persistent == 1 and info.launches == 1 and info.temporal_depth == 8, what
            if entered != expected:
                msgs.append(f"{what}: {entered} waves entered scaled mode, exactly {expected} expected")
            try:
                assert_bit_equal_nan_aware(down(d), want, what)
            except AssertionError as e:
                msgs.append(str(e))
    finally:
        ctx.set_option(rt.OPT_FP_CONTRACT, 1); ctx.set_option(rt.OPT_PERSISTENT, 1)
        for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH):
            ctx.set_option(k, 0)
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs[:12])
