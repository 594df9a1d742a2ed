"""The solver family on depth maps outside [0, 255] (-m gpu): negative, huge, infinite and NaN depths (tests/wild_depth.py) through every
sweep kernel, the gated edge-weight rule, red-black, the residual stop, multigrid, the cascade's pieces and a whole estimate, each
against the oracle or the existing restatements.  The bits must be the reference's arithmetic for EVERY f32 depth; only a NaN's sign
and payload are left out (gpu_util.assert_bit_equal_nan_aware).  tests/test_wild_depth_cpu.py shows, on the oracle alone, that the
classes with +inf or overflowing sums can tell a divide that answers NaN (clamped to 0) from the IEEE quotient (+inf, clamped to 255)."""
import ctypes as C

import numpy as np
import pytest

import realtimedepthdiffusion_amd as rt
import wild_depth as wd
from cascade_ref import Cascade
from gpu_util import assert_bit_equal_nan_aware, down, up
from test_gpu_cascade import _bgr

pytestmark = pytest.mark.gpu

NAMES = sorted(wd.CLASSES)
FULL = ("huge", "infinite_on_dirichlet")          # these two meet every kernel configuration below; the others one of each family
LEVELS = [(0, 1), (1, 3)]                         # (level, levels): un-gated weights; the gated rule, which reads the wild depth

K = rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH, rt.OPT_PERSISTENT


def _k2(tile, depth, persistent):
    return {rt.OPT_SWEEP_KERNEL: 2, rt.OPT_TILE: tile, rt.OPT_TEMPORAL_DEPTH: depth, rt.OPT_PERSISTENT: persistent}


# kernel families: one sweep per launch; the blocked kernel's row layout (tile 1), its 1024-thread tile (3), its 24-pixels-per-thread
# tile (13), the column layout (14, 16); the automatic choice.  Temporal depths 1, 4 and 8, launch per block and persistent.
FAMILIES = {
    "one_sweep": [{rt.OPT_SWEEP_KERNEL: 1}],
    "auto": [{}, {rt.OPT_PERSISTENT: 0}],
    "row": [_k2(1, 1, 0), _k2(1, 4, 0), _k2(1, 4, 1), _k2(1, 8, 1), _k2(1, 8, 0)],
    "wide": [_k2(3, 4, 0), _k2(3, 8, 1), _k2(3, 1, 0)],
    "deep": [_k2(13, 8, 0), _k2(13, 4, 1), _k2(13, 1, 0)],
    "column": [_k2(14, 1, 0), _k2(14, 4, 0), _k2(14, 8, 0), _k2(16, 4, 0), _k2(16, 8, 0), _k2(16, 1, 0)],
}


def _configs(name, salt):
    if name in FULL:
        return [(f, o) for f, group in FAMILIES.items() for o in group]
    return [(f, group[(NAMES.index(name) + salt) % len(group)]) for f, group in FAMILIES.items()]


@pytest.fixture(scope="module")
def _ctx():
    c = rt.Context(0)
    c.GPULoadWeights(0.4)
    yield c
    c.close()


@pytest.fixture
def ctx(_ctx):
    """The shared context with every option back at its default."""
    _ctx.set_option(rt.OPT_FP_CONTRACT, 1); _ctx.set_option(rt.OPT_PERSISTENT, 1)
    for k in (rt.OPT_SWEEP_KERNEL, rt.OPT_TILE, rt.OPT_TEMPORAL_DEPTH, rt.OPT_ROWS_PER_WAVE):
        _ctx.set_option(k, 0)
    return _ctx


def _set(ctx, opts):
    for k in K:
        ctx.set_option(k, opts.get(k, 1 if k == rt.OPT_PERSISTENT else 0))


class Failures:
    """Every mismatch of a test is reported, not only the first: which kernels part from the oracle is what one wants to know."""

    def __init__(self):
        self.msgs = []

    def check(self, got, want, what):
        try:
            assert_bit_equal_nan_aware(got, want, what)
        except AssertionError as e:
            self.msgs.append(str(e))

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} mismatches:\n" + "\n".join(self.msgs[:12])


@pytest.mark.parametrize("shape", wd.JACOBI_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NAMES)
def test_jacobi_every_kernel(ctx, oracle, lut, name, shape):
    """rtdd_matrix_free_solver and rtdd_solve_ex, 1, 2, 7 and 24 sweeps (24 is no multiple of depth 7 or 8; depth 4 runs several
    launches), both contractions, both level rules, 512-aligned and 4-aligned images (k_prepare4 and k_prepare): equal to the oracle,
    and the one-sweep kernel and every blocked configuration equal to each other."""
    rows, cols = shape
    p = wd.make(name, rows, cols)
    fails = Failures()
    turn = 0
    for level, levels in LEVELS:
        ctx.GPUAllocateDeviceMemory(rows << level, cols << level, levels)
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            want = {n: oracle.solve(p["depth"].copy(), p["mask"], p["gray"], n, level, levels - 1, lut, contract) for n in wd.JACOBI_SWEEPS}
            images = {a: (up(p["mask"], a), up(p["gray"], a)) for a in (512, 4)}
            one_sweep = {}
            for family, opts in _configs(name, rows + level + contract):
                _set(ctx, opts)
                for n in wd.JACOBI_SWEEPS:
                    turn += 1
                    align = (512, 4)[turn % 2]
                    m, g = images[align]
                    d = up(p["depth"], align)
                    if (turn // 2) % 2:
                        ctx.GPUMatrixFreeSolver(d, m, g, rows, cols, 0.4, n, 1e-5, level)
                    else:
                        its, _ = ctx.solve_ex(d, m, g, rows, cols, level, method=rt.METHOD_CHEBYSHEV_JACOBI, maxIterations=n, tolerance=0.0)
                        assert its == n
                    ctx.synchronize()
                    got = down(d)
                    info = ctx.last_solve_info()
                    if family == "one_sweep":
                        assert info.kernel == 1, info.describe()
                        one_sweep[n] = got
                    elif family != "auto":
                        assert info.kernel == 2 and info.tile == opts[rt.OPT_TILE], info.describe()
                    what = f"{name} {rows}x{cols} level {level}/{levels} contract {contract} align {align} x{n} [{info.describe()}]"
                    fails.check(got, want[n], "oracle: " + what)
                    if family != "one_sweep":
                        fails.check(got, one_sweep[n], "kernel 1 against this kernel: " + what)
    fails.done()


@pytest.mark.parametrize("name", NAMES)
def test_edge_weights(ctx, oracle, name):
    """rtdd_index_to_weight at (level, levels) = (1, 3) and (2, 3): the gated rule's saturating float -> u8 of a wild depth."""
    import torch
    for rows, cols in wd.JACOBI_SHAPES:
        p = wd.make(name, rows, cols)
        for level in (1, 2):
            ctx.GPUAllocateDeviceMemory(rows << level, cols << level, 3)
            for align in (512, 4):
                idx = torch.zeros((rows, cols, 2), dtype=torch.int32, device="cuda:0")
                ctx.index_to_weight(up(p["gray"], align), up(p["depth"], align), idx, level, rows, cols)
                ctx.synchronize()
                want = oracle.index_to_weight(p["gray"], p["depth"], level, 2)
                assert np.array_equal(idx.cpu().numpy(), want), f"{name} {rows}x{cols} level {level}/3 align {align}"


@pytest.mark.parametrize("shape", wd.RED_BLACK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NAMES)
def test_red_black(ctx, oracle, lut, name, shape):
    """RTDD_METHOD_RED_BLACK_GS, relaxation 1.0, 1.7 and 1.93, 1, 5 and 12 sweeps, both contractions, the one-colour-per-launch kernel
    and the register-blocked one (both tile shapes), against the oracle's in-place sweep."""
    rows, cols = shape
    p = wd.make(name, rows, cols)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    m, g = up(p["mask"]), up(p["gray"])
    fails = Failures()
    for contract in (1, 0):
        ctx.set_option(rt.OPT_FP_CONTRACT, contract)
        for omega in (1.0, 1.7, 1.93):
            for sweeps in (1, 5, 12):
                x = p["depth"].copy()
                for _ in range(sweeps):
                    oracle.rbgs_sweep(x, idx, p["mask"], lut, contract, omega)
                for kernel, tile, depth in ((0, 0, 0), (1, 0, 0), (0, 1, 4), (0, 2, 5)):
                    ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel); ctx.set_option(rt.OPT_TILE, tile); ctx.set_option(rt.OPT_TEMPORAL_DEPTH, depth)
                    d = up(p["depth"])
                    its, _ = ctx.solve_ex(d, m, g, rows, cols, 0, method=rt.METHOD_RED_BLACK_GS, maxIterations=sweeps, tolerance=0.0, relaxation=omega)
                    ctx.synchronize()
                    info = ctx.last_solve_info()
                    # (kernel 3: one launch per colour; 4: register-blocked, where an image that fits one 128 x 128 tile always takes tile 2)
                    assert its == sweeps and info.kernel == (3 if kernel == 1 else 4), info.describe()
                    assert kernel == 1 or tile == 0 or (rows <= 128 and cols <= 128) or info.tile == tile, info.describe()
                    fails.check(down(d), x, f"rbgs {name} {rows}x{cols} contract {contract} omega {omega} x{sweeps} [{info.describe()}]")
    fails.done()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name", ["out_of_range", "nan", "infinite"])
def test_residual_stop(ctx, oracle, lut, name, kernel):
    """rtdd_solve_ex with tolerance 1e-4, checkEvery 16, maxIterations 64: (iterations, residual) and the bits equal the restated loop
    over oracle.solve and oracle.residual -- which fixes how a NaN or infinite pixel enters max|J(x) - x|: a NaN difference counts
    as +inf (include/rtdd.h), so such a map never passes for converged."""
    for rows, cols in [(70, 133), (24, 24)]:
        p = wd.make(name, rows, cols)
        ctx.GPUAllocateDeviceMemory(rows, cols, 1)
        ctx.set_option(rt.OPT_SWEEP_KERNEL, kernel)
        idx = oracle.index_to_weight(p["gray"], None, 0, 0)
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            for want_its in (16, 32, 48, 64):
                x = oracle.solve(p["depth"].copy(), p["mask"], p["gray"], want_its, 0, 0, lut, contract)
                want_res = np.float32(oracle.residual(x, idx, p["mask"], lut, contract))
                if want_res <= np.float32(1e-4):
                    break
            d = up(p["depth"])
            its, res = ctx.solve_ex(d, up(p["mask"]), up(p["gray"]), rows, cols, 0, method=rt.METHOD_CHEBYSHEV_JACOBI, maxIterations=64, tolerance=1e-4, checkEvery=16)
            ctx.synchronize()
            what = f"{name} {rows}x{cols} contract {contract} kernel {kernel}"
            print(f"{what}: GPU ({its}, {res!r}), restated ({want_its}, {want_res!r})")
            assert its == want_its, what
            assert_bit_equal_nan_aware(np.float32([res]), np.float32([want_res]), "residual: " + what)
            assert_bit_equal_nan_aware(down(d), x, what)


@pytest.mark.parametrize("rows,cols", [(75, 133), (33, 7)])
@pytest.mark.parametrize("name", ["out_of_range", "magnitudes", "nan", "infinite"])
def test_multigrid(ctx, oracle, lut, name, rows, cols):
    """2 V-cycles, both contractions, against oracle.mg_solve."""
    p = wd.make(name, rows, cols)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    fails = Failures()
    for contract in (1, 0):
        ctx.set_option(rt.OPT_FP_CONTRACT, contract)
        x = p["depth"].copy()
        oracle.mg_solve(x, idx, p["mask"], lut, contract, 2, 0.0, 1)
        d = up(p["depth"])
        its, _ = ctx.solve_ex(d, up(p["mask"]), up(p["gray"]), rows, cols, 0, method=rt.METHOD_MULTIGRID, maxIterations=2, tolerance=0.0)
        ctx.synchronize()
        assert its == 2
        fails.check(down(d), x, f"multigrid {name} {rows}x{cols} contract {contract}")
    fails.done()


def test_auto_method_out_of_range(ctx, oracle, lut):
    """One RTDD_METHOD_AUTO solve from an out-of-range start: cycle count, sweep count, residual and bits as the same logic driven
    through the restatements (as test_auto_method_vcycles_then_sor_cycles does from the cold start)."""
    from test_gpu_parity import _sor_cycles_restated
    rows, cols = 75, 133
    p = wd.make("out_of_range", rows, cols)
    ctx.GPUAllocateDeviceMemory(rows, cols, 1)
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    d = up(p["depth"])
    its, res = ctx.solve_ex(d, up(p["mask"]), up(p["gray"]), rows, cols, 0, method=rt.METHOD_AUTO, maxIterations=300, tolerance=1e-4)
    ctx.synchronize()
    cycles = ctx.last_cycles
    x = p["depth"].copy()
    sor_seconds, cycle_seconds = ctx.auto_model(rows, cols)
    want_cycles, want_res, _ = oracle.mg_solve(x, idx, p["mask"], lut, 1, 60, 1e-4, 1, alternative_seconds=sor_seconds, cycle_seconds=cycle_seconds)
    want_its = 0
    if not want_res <= 1e-4:
        want_its, want_res = _sor_cycles_restated(oracle, x, idx, p["mask"], lut, 1, 1e-4, 300, halve=True)
    print(f"auto: GPU ({cycles}, {its}, {res!r}), restated ({want_cycles}, {want_its}, {np.float32(want_res)!r})")
    assert (cycles, its) == (want_cycles, want_its)
    assert_bit_equal_nan_aware(np.float32([res]), np.float32([want_res]), "residual")
    assert_bit_equal_nan_aware(down(d), x, "auto")


@pytest.mark.parametrize("name", NAMES)
def test_pyrup_depth(ctx, oracle, name):
    """rtdd_pyrup_depth: exact doubling through the four-pixel kernel (8x10 -> 16x20) and the scalar one (7x9 -> 14x18), and the
    explicit-size branch (7x9 -> 13x17, 1x5 -> 1x9), both contractions, against the cascade restatement."""
    fails = Failures()
    for (rows, cols), (drows, dcols) in (((8, 10), (16, 20)), ((7, 9), (14, 18)), ((7, 9), (13, 17)), ((1, 5), (1, 9))):
        src = wd.make(name, rows, cols)["depth"]
        for contract in (1, 0):
            ctx.set_option(rt.OPT_FP_CONTRACT, contract)
            for align in (512, 4):
                dst = up(np.zeros((drows, dcols), np.float32), align)
                ctx.pyrup_depth(up(src, align), rows, cols, dst, drows, dcols)
                ctx.synchronize()
                fails.check(down(dst), oracle.pyrup_f32(src, drows, dcols, contract=contract), f"pyrUp {name} {rows}x{cols} -> {drows}x{dcols} contract {contract} align {align}")
    fails.done()


def test_depth_to_u8_table(ctx):
    """rtdd_depth_to_u8 against saturate(rint) written in numpy, NaN -> 0: every tie, the ends of the range, the specials, denormals."""
    f = np.float32
    around = [np.nextafter(f(v), f(s)) for v in (0, 0.5, 254.5, 255) for s in (-np.inf, np.inf)]
    v = np.concatenate([np.arange(-2, 257, dtype=np.float32) + f(0.5),
                        f([0.0, -0.0, np.inf, -np.inf, np.nan, 1e10, -1e10, 254.49999, 255.5, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38]), f(around)])
    v = np.ascontiguousarray(v[None, :])
    for align in (512, 4):
        u = up(np.full(v.shape, 77, np.uint8), align)
        ctx.depth_to_u8(up(v, align), u, 1, v.shape[1])
        ctx.synchronize()
        got, want = down(u), wd.round_u8(v)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, [(float(v[0, i]), int(got[0, i]), int(want[0, i])) for i in bad[:8]]


def _estimate_single(oracle, lut, rows, cols, bgr, ann, start, sweeps, fails):
    """One estimate from `start` uploaded into the coarsest RTDD_IMG_DEPTH, checked against the cascade restatement; returns the maps."""
    ref = Cascade(oracle, bgr, ann, lut, 1, threads=min(4, oracle.max_threads()))
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        P = c.pyramid_create(rows, cols)
        assert P == ref.P and P >= 2
        c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
        _upload_coarsest(c, P, start)
        ref.depth[P - 1][...] = start
        ref.estimate(sweeps); c.estimate_depth(sweeps); c.synchronize()
        maps = [c.pyramid_download(rt.IMG_DEPTH, l) for l in range(P)]
        u8 = c.pyramid_download(rt.IMG_DEPTH_U8)
    return ref, maps, u8


def _upload_coarsest(c, P, start):
    ptr, pitch, lr, lc = c.pyramid_image(rt.IMG_DEPTH, P - 1)
    assert (lr, lc) == start.shape
    host = np.ascontiguousarray(start)
    c._check(rt.lib().rtdd_upload(c._h, C.c_void_p(ptr), C.c_size_t(pitch), C.c_void_p(host.ctypes.data), C.c_size_t(lc * 4), C.c_size_t(lc * 4), C.c_int(lr)))


def _coarsest_shape(rows, cols):
    from cascade_ref import pyramid_levels
    P = pyramid_levels(rows, cols)
    return int(np.float32(rows) / np.float32(2.0) ** (P - 1)), int(np.float32(cols) / np.float32(2.0) ** (P - 1))


@pytest.mark.parametrize("name", ["magnitudes", "infinite", "nan"])
@pytest.mark.parametrize("rows,cols", [(90, 91), (135, 241)])
def test_whole_estimate(oracle, lut, rows, cols, name):
    """A wild map uploaded into the coarsest RTDD_IMG_DEPTH, then rtdd_estimate_depth with 50 sweeps per level: RTDD_IMG_DEPTH of every
    level equals cascade_ref.Cascade on the same start, and RTDD_IMG_DEPTH_U8 the u8 rule applied to the level-0 map.  The finer
    levels start from what the pyrUp-and-inject kernel made of the coarse result (NaN and +-inf spread by its 5 x 5 footprint): each
    level's own k_prepare has to notice them again."""
    bgr, ann = _bgr(rows, cols, 11)
    start = wd.make(name, *_coarsest_shape(rows, cols))["depth"]
    fails = Failures()
    ref, maps, u8 = _estimate_single(oracle, lut, rows, cols, bgr, ann, start, 50, fails)
    for l in range(ref.P - 1, -1, -1):
        fails.check(maps[l], ref.depth[l], f"{name} {rows}x{cols} depth level {l}")
    fails.done()
    assert np.array_equal(u8, wd.round_u8(maps[0])), "RTDD_IMG_DEPTH_U8 is not saturate(rint) of the level-0 map"
    assert np.array_equal(u8, ref.depth_u8)


def test_whole_estimate_batch(oracle, lut):
    """A batch of 3 with a different class per image: each image equals its single-image result."""
    rows, cols = 90, 91
    names = ["magnitudes", "infinite", "nan"]
    data = [_bgr(rows, cols, 40 + b) for b in range(3)]
    starts = [wd.make(n, *_coarsest_shape(rows, cols))["depth"] for n in names]
    fails = Failures()
    singles = [_estimate_single(oracle, lut, rows, cols, bgr, ann, s, 50, fails) for (bgr, ann), s in zip(data, starts)]
    with rt.Context(0) as c:
        c.GPULoadWeights(0.4)
        P = c.pyramid_create_batch(rows, cols, 3)
        for b, (bgr, ann) in enumerate(data):
            c.pyramid_select(b); c.pyramid_set_image(up(bgr)); c.pyramid_set_annotation(up(ann))
            _upload_coarsest(c, P, starts[b])
        c.estimate_depth_batch(50); c.synchronize()
        for b, (ref, maps, u8) in enumerate(singles):
            c.pyramid_select(b)
            for l in range(P):
                got = c.pyramid_download(rt.IMG_DEPTH, l)
                fails.check(got, maps[l], f"image {b} ({names[b]}) level {l}: batch against single")
                fails.check(got, ref.depth[l], f"image {b} ({names[b]}) level {l}: batch against the restatement")
            assert np.array_equal(c.pyramid_download(rt.IMG_DEPTH_U8), u8), f"image {b} u8"
    fails.done()
