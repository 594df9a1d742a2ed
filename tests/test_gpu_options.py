"""rtdd_set_option / rtdd_get_option (include/rtdd.h) through the C ABI (-m gpu: a context needs a device; no kernel is launched).  The
ranges and refusal texts below are written out by hand from the library's behaviour before the options became one table: the test is a
statement about what a caller sees, not about the table.  Every key of the header's enum is covered -- a new option has to be added
here."""
import ctypes as C
import os
import re

import pytest

import realtimedepthdiffusion_amd as rt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                     # RTDD_ERR_INVALID
INT_MAX, INT_MIN = 2**31 - 1, -2**31

# key -> (lowest, highest admitted value (None: no upper bound below INT_MAX), refusal text)
RANGED = {
    rt.OPT_SWEEP_KERNEL: (0, 2, "sweep kernel must be 0..2"),
    rt.OPT_TEMPORAL_DEPTH: (0, 28, "temporal depth must be 0..28"),
    rt.OPT_DEFOCUS_PATH: (0, 2, "defocus path must be 0..2"),
    rt.OPT_ROWS_PER_WAVE: (0, 1024, "rows per wave must be 0..1024"),
    rt.OPT_TILE: (0, 16, "tile must be 0..16"),
    rt.OPT_DEBUG_WITHHOLD_TILE: (0, 1024, "tile number + 1 out of range"),
    rt.OPT_DEBUG_POLL_LIMIT_US: (0, 10000000, "poll limit must be 0..1e7 us"),
    rt.OPT_AUTO_CYCLE_FIXED_NS: (0, None, "must be >= 0"),
    rt.OPT_AUTO_CYCLE_FS_PER_PX: (0, None, "must be >= 0"),
    rt.OPT_AUTO_SWEEP_FS_PER_PX: (0, None, "must be >= 0"),
    rt.OPT_AUTO_SWEEP_FLOOR_NS: (0, None, "must be >= 0"),
    rt.OPT_DEBUG_FORCE_STATUS: (0, 3, "status must be 0..3"),
    rt.OPT_PERSISTENT_REARM_AFTER: (0, 1 << 20, "must be 0..2^20"),
    rt.OPT_LIVE_ZERO_COPY: (0, 2, "RTDD_OPT_LIVE_ZERO_COPY is 0, 1 or 2"),
    rt.OPT_DEFOCUS_STRIPS: (0, 2, "must be 0, 1 or 2"),
    rt.OPT_DEFOCUS_SLICE_MB: (0, 4095, "must be 0..4095 MB"),
}
ZERO_OR_ONE = [rt.OPT_FP_CONTRACT, rt.OPT_PERSISTENT, rt.OPT_TIMEOUT_HEAL, rt.OPT_ANNOTATION_LDS]
READ_ONLY = [rt.OPT_TIMEOUT_HEALS, rt.OPT_DEFOCUS_LAST_PATH, rt.OPT_PERSISTENT_SUSPENDED, rt.OPT_PENDING_CALLS, rt.OPT_DEFOCUS_LAST_SLICES]


class Raw:
    """The two calls and rtdd_last_error on one context's handle, statuses returned and not raised."""

    def __init__(self, ctx):
        self.h, self.L = ctx._h, rt.lib()

    def set(self, key, value):
        return self.L.rtdd_set_option(self.h, C.c_int(key), C.c_int(value))

    def get(self, key):
        v = C.c_int(-12345)
        return self.L.rtdd_get_option(self.h, C.c_int(key), C.byref(v)), v.value

    def error(self):
        return self.L.rtdd_last_error(self.h).decode()


@pytest.fixture()
def raw():
    c = rt.Context(0)
    yield Raw(c)
    c.close()


def test_the_table_above_covers_the_header(raw):
    text = open(os.path.join(ROOT, "include", "rtdd.h")).read()
    header = {int(v) for v in re.findall(r"^\s*RTDD_OPT_\w+\s*=\s*(\d+)", text, re.M)}
    assert header == set(range(25))
    assert sorted(list(RANGED) + ZERO_OR_ONE + READ_ONLY) == sorted(header)


@pytest.mark.parametrize("key", sorted(RANGED))
def test_a_ranged_option_takes_its_range_and_refuses_the_rest(raw, key):
    lo, hi, text = RANGED[key]
    for v in (lo, hi if hi is not None else INT_MAX):
        assert raw.set(key, v) == rt.RTDD_OK
        assert raw.get(key) == (rt.RTDD_OK, v)
    assert raw.set(key, lo + 1) == rt.RTDD_OK
    for bad in [lo - 1, INT_MIN] + ([hi + 1, INT_MAX] if hi is not None else []):
        assert raw.set(key, bad) == INVALID
        assert raw.error() == text
        assert raw.get(key) == (rt.RTDD_OK, lo + 1)             # unchanged


@pytest.mark.parametrize("key", ZERO_OR_ONE)
def test_a_zero_or_one_option_normalises(raw, key):
    assert raw.get(key) == (rt.RTDD_OK, 1)                      # all four default to 1
    for v, want in ((0, 0), (1, 1), (0, 0), (7, 1), (0, 0), (-1, 1), (INT_MIN, 1)):
        assert raw.set(key, v) == rt.RTDD_OK
        assert raw.get(key) == (rt.RTDD_OK, want)


@pytest.mark.parametrize("key", READ_ONLY)
def test_a_read_only_key_reads_and_refuses_a_set(raw, key):
    assert raw.get(key) == (rt.RTDD_OK, 0)                      # a fresh context: no heal, no defocus, nothing suspended or pending
    for v in (0, 1):
        assert raw.set(key, v) == INVALID
        assert raw.error() == "unknown option"
    assert raw.get(key) == (rt.RTDD_OK, 0)


@pytest.mark.parametrize("key", [25, -1])
def test_an_unknown_key_is_refused_both_ways(raw, key):
    assert raw.set(key, 0) == INVALID
    assert raw.error() == "unknown option"
    raw.set(rt.OPT_TILE, 99)                                    # (another text in between)
    assert raw.get(key) == (INVALID, -12345)                    # (the caller's value is left alone)
    assert raw.error() == "unknown option"


def test_null_arguments(raw):
    L = raw.L
    assert L.rtdd_set_option(None, C.c_int(rt.OPT_TILE), C.c_int(0)) == INVALID
    assert L.rtdd_get_option(None, C.c_int(rt.OPT_TILE), C.byref(C.c_int())) == INVALID
    assert L.rtdd_get_option(raw.h, C.c_int(rt.OPT_TILE), None) == INVALID


def test_the_side_effects_that_show_without_a_kernel(raw):
    for v in (1, 0, 7):
        assert raw.set(rt.OPT_PERSISTENT, v) == rt.RTDD_OK
        assert raw.get(rt.OPT_PERSISTENT_SUSPENDED) == (rt.RTDD_OK, 0)
    assert raw.set(rt.OPT_TIMEOUT_HEAL, 0) == rt.RTDD_OK
    assert raw.get(rt.OPT_PENDING_CALLS) == (rt.RTDD_OK, 0)
    assert raw.set(rt.OPT_DEFOCUS_PATH, 0) == rt.RTDD_OK
    assert raw.get(rt.OPT_DEFOCUS_LAST_PATH) == (rt.RTDD_OK, 0)


def test_the_defaults(raw):
    want = {rt.OPT_SWEEP_KERNEL: 0, rt.OPT_TEMPORAL_DEPTH: 0, rt.OPT_DEFOCUS_PATH: 0, rt.OPT_ROWS_PER_WAVE: 0, rt.OPT_TILE: 0,
            rt.OPT_DEBUG_WITHHOLD_TILE: 0, rt.OPT_DEBUG_POLL_LIMIT_US: 0, rt.OPT_AUTO_CYCLE_FIXED_NS: 270000,
            rt.OPT_AUTO_CYCLE_FS_PER_PX: 46000, rt.OPT_AUTO_SWEEP_FS_PER_PX: 1429, rt.OPT_AUTO_SWEEP_FLOOR_NS: 2500,
            rt.OPT_DEBUG_FORCE_STATUS: 0, rt.OPT_PERSISTENT_REARM_AFTER: 64, rt.OPT_LIVE_ZERO_COPY: 1, rt.OPT_DEFOCUS_STRIPS: 0,
            rt.OPT_DEFOCUS_SLICE_MB: 0}
    assert set(want) == set(RANGED)
    for key, v in want.items():
        assert raw.get(key) == (rt.RTDD_OK, v)
