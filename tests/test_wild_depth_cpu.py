"""The input classes of tests/wild_depth.py, checked on the oracle alone (no GPU): that they leave most of the result finite, so that a
comparison on them compares numbers; that the classes with +inf or overflowing sums can tell a divide that answers NaN (clamped to 0)
from the IEEE quotient (+inf, clamped to 255); and that the NaN-aware comparison treats NaN, +-0 and +-inf as it says."""
import warnings

import numpy as np
import pytest

import wild_depth as wd
from gpu_util import assert_bit_equal, assert_bit_equal_nan_aware

LEVELS = [(0, 1), (1, 3)]            # (level, levels): un-gated weights; the gated rule, which reads the wild depth
RB_SHAPES = wd.RED_BLACK_SHAPES
MG_SHAPES = [(75, 133), (33, 7)]


def _jacobi(oracle, lut, p, depth, sweeps, level, levels, contract=1):
    return oracle.solve(depth.copy(), p["mask"], p["gray"], sweeps, level, levels - 1, lut, contract, threads=min(4, oracle.max_threads()))


def _rbgs(oracle, lut, p, depth, sweeps, omega, contract=1):
    idx = oracle.index_to_weight(p["gray"], None, 0, 0)
    x = depth.copy()
    for _ in range(sweeps):
        oracle.rbgs_sweep(x, idx, p["mask"], lut, contract, omega)
    return x


def _finite_share_of_free(p, result):
    free = p["mask"] != 255
    return float(np.isfinite(result[free]).mean()) if free.any() else 1.0


@pytest.mark.parametrize("name", sorted(wd.CLASSES))
def test_classes_are_what_they_say(name):
    for rows, cols in wd.JACOBI_SHAPES:
        p = wd.make(name, rows, cols)
        d, lab = p["depth"], p["mask"] == 255
        assert (~lab).sum() * 2 >= lab.size and lab.any(), "a class needs free pixels and a label"
        q = wd.make(name, rows, cols)
        assert_bit_equal_nan_aware(q["depth"], d, "the same seed gives the same map")
        special = ~np.isfinite(d) | (np.abs(np.nan_to_num(d)) >= 1e38)
        if name.endswith("_on_dirichlet"):
            assert special.any() and not special[~lab].any() and (d[~lab] >= 0).all() and (d[~lab] <= 255).all()
        elif name.endswith("_at_edges"):
            y, x = np.nonzero(special)
            on_edge = (y == 0) | (y == rows - 1) | (x == 0) | (x == cols - 1) | np.isin(y, wd.TILE_EDGES) | np.isin(x, wd.TILE_EDGES)
            assert special.any() and on_edge.all()
        elif name in ("huge", "infinite", "nan"):
            assert special[~lab].any() and not special[lab].any()
        elif name == "out_of_range":
            assert np.isfinite(d).all() and (d[~lab] >= -300).all() and (d[~lab] <= 600).all()
            if rows * cols > 100:
                assert d[~lab].min() < -100 and d[~lab].max() > 400
                for v in (np.float32(-0.0), np.float32(255), np.float32(256), np.float32(-1)):
                    assert (d.view(np.uint32) == v.view(np.uint32)).any(), v
        else:
            a = np.abs(d[~lab])
            assert np.isfinite(d).all() and a.max() <= 1.0001e30 and a.min() >= 0.9999e-30 and (d[~lab] < 0).any() and (d[~lab] > 0).any()
        if name.startswith("infinite"):
            assert np.isposinf(d).any() and np.isneginf(d).any()
        if name.startswith("nan"):
            assert np.isnan(d).any() and not np.isinf(d).any()


@pytest.mark.parametrize("level,levels", LEVELS)
@pytest.mark.parametrize("name", sorted(wd.CLASSES))
def test_most_free_pixels_stay_finite_under_jacobi(oracle, lut, name, level, levels):
    """Condition (a): after the largest sweep count the tests use, at least half of the free pixels of the oracle's result are finite (a
    NaN pixel stays NaN, but clamp255 keeps it out of its neighbours' means)."""
    for rows, cols in wd.JACOBI_SHAPES:
        p = wd.make(name, rows, cols)
        got = _jacobi(oracle, lut, p, p["depth"], max(wd.JACOBI_SWEEPS), level, levels)
        assert _finite_share_of_free(p, got) >= 0.5, (name, rows, cols)


@pytest.mark.parametrize("name", sorted(wd.CLASSES))
def test_most_free_pixels_stay_finite_under_red_black_and_multigrid(oracle, lut, name):
    for rows, cols in RB_SHAPES:
        p = wd.make(name, rows, cols)
        for omega in (1.0, 1.93):
            assert _finite_share_of_free(p, _rbgs(oracle, lut, p, p["depth"], 12, omega)) >= 0.5, (name, rows, cols, omega)
    if name in ("out_of_range", "magnitudes", "nan", "infinite"):
        for rows, cols in MG_SHAPES:
            p = wd.make(name, rows, cols)
            x = p["depth"].copy()
            oracle.mg_solve(x, oracle.index_to_weight(p["gray"], None, 0, 0), p["mask"], lut, 1, 2, 0.0, 1)
            assert _finite_share_of_free(p, x) >= 0.5, (name, rows, cols)


@pytest.mark.parametrize("level,levels", LEVELS)
@pytest.mark.parametrize("sweeps", wd.JACOBI_SWEEPS)
@pytest.mark.parametrize("name", wd.OVERFLOWING)
def test_overflow_classes_can_see_a_nan_for_an_infinite_quotient(oracle, lut, name, sweeps, level, levels):
    """Condition (b): the oracle's result on the input differs, in a pixel finite on both sides, from its result with every +inf (for
    `huge`: every value >= 1e38) replaced by NaN -- which is what a divide that answers NaN to such a numerator computes.  So a kernel
    with that fault cannot pass a comparison on these inputs."""
    for rows, cols in wd.JACOBI_SHAPES:
        p = wd.make(name, rows, cols)
        a = _jacobi(oracle, lut, p, p["depth"], sweeps, level, levels)
        b = _jacobi(oracle, lut, p, wd.overflow_as_nan(name, p["depth"]), sweeps, level, levels)
        n = int(wd.finite_on_both_and_different(a, b).sum())
        assert n >= 1, f"{name} {rows}x{cols} x{sweeps} level {level}/{levels}: the input cannot tell NaN -> 0 from +inf -> 255"


@pytest.mark.parametrize("name", wd.OVERFLOWING)
def test_overflow_classes_can_see_it_under_red_black_too(oracle, lut, name):
    """Condition (b) for the in-place sweep.  A Gauss-Seidel update REPLACES a free +inf pixel by its neighbours' mean, so what it did to
    them is all that is left of it, and on a 7-pixel image a clamped over-relaxed step can erase even that within a few sweeps: there the
    longer runs are asked of the classes whose special values sit on Dirichlet pixels, which never change; the first sweep of all."""
    for rows, cols in RB_SHAPES:
        p = wd.make(name, rows, cols)
        for sweeps, omega in ((1, 1.0), (5, 1.7), (12, 1.93)):
            if sweeps > 1 and rows * cols < 100 and not name.endswith("_on_dirichlet"):
                continue
            a = _rbgs(oracle, lut, p, p["depth"], sweeps, omega)
            b = _rbgs(oracle, lut, p, wd.overflow_as_nan(name, p["depth"]), sweeps, omega)
            assert wd.finite_on_both_and_different(a, b).any(), (name, rows, cols, sweeps, omega)


def test_nan_aware_comparison():
    """Condition (c)."""
    f = lambda *v: np.array(v, np.float32)
    qnan, other = np.uint32(0x7FC00000).view(np.float32), np.uint32(0xFFC12345).view(np.float32)     # x86's default NaN; a negative one with a payload
    assert_bit_equal_nan_aware(f(qnan, 1.0, -0.0, np.inf), f(other, 1.0, -0.0, np.inf))
    with pytest.raises(AssertionError), np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (its message takes a nanmax of nothing but NaN)
        assert_bit_equal(f(qnan), f(other))                            # the strict helper keeps its meaning
    for got, want in ((f(0.0), f(-0.0)), (f(np.inf), f(-np.inf)), (f(np.nan), f(0.0)), (f(np.nan), f(np.inf)), (f(1.0), f(np.nextafter(np.float32(1), np.float32(2))))):
        with pytest.raises(AssertionError):
            assert_bit_equal_nan_aware(got, want)
    with pytest.raises(AssertionError) as e:
        assert_bit_equal_nan_aware(f(np.nan, 0.0, 3.0, np.inf, 7.0), f(np.nan, -0.0, 3.0, 255.0, 7.5), "msg")
    text = str(e.value)
    assert "msg: 3 of 5 values differ, 2 of them finite on both sides; first at (1,)" in text and "0x00000000" in text and "0x80000000" in text
    with pytest.raises(AssertionError):
        assert_bit_equal_nan_aware(np.zeros((2, 3), np.float32), np.zeros((3, 2), np.float32))


def test_round_u8_restatement_is_the_oracle_rule(oracle):
    v = np.concatenate([np.arange(-2, 257, dtype=np.float32) + np.float32(0.5), np.random.default_rng(3).uniform(-10, 300, 500).astype(np.float32),
                        np.array([np.inf, -np.inf, np.nan, 1e10, -1e10, 254.49999, 255.5, 0.0, -0.0], np.float32)])[None, :]
    assert np.array_equal(wd.round_u8(v), oracle.depth_to_u8(np.ascontiguousarray(v)))
