"""tests/roi_util.py tested without a GPU: the two checkers on a numpy stand-in for the parent.  A single changed byte planted in the right
padding, the lead, a guard row above, a guard row below and inside an input view is reported with its position; a clean parent passes."""
import numpy as np
import pytest

from roi_util import (FILL_INPUT, FILL_OUTPUT, GUARD_BYTES, GUARD_ROWS, LAYOUTS_F32, LAYOUTS_U8, Roi, covering, pitch_for)


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (5, 7), dtype=np.uint8), rng.integers(0, 256, (3, 6, 3), dtype=np.uint8),
            rng.uniform(0, 255, (4, 9)).astype(np.float32), rng.integers(0, 256, (1, 1), dtype=np.uint8)]


def _layouts(host):
    w = host.size // host.shape[0] * host.itemsize
    return [(lead, pitch_for(w, lead, res)) for lead, res in (LAYOUTS_F32 if host.dtype == np.float32 else LAYOUTS_U8)]


def test_the_layout_lists_cover_the_alignment_classes():
    assert {l for l, _ in LAYOUTS_U8} == {0, 1, 2, 3, 4} and {l for l, _ in LAYOUTS_F32} == {0, 4, 8, 12}
    for w in (7, 21, 36, 259 * 3):
        pu = [pitch_for(w, l, r) for l, r in LAYOUTS_U8]
        assert {p % 4 for p in pu} == {0, 1, 2, 3} and any(p % 16 == 0 for p in pu)
        pf = [pitch_for(w // 4 * 4, l, r) for l, r in LAYOUTS_F32]
        assert {p % 16 for p in pf} == {0, 4, 8, 12}
    assert (1, 0) in LAYOUTS_U8 and (0, 1) in LAYOUTS_U8          # an aligned pitch under an unaligned base, and the reverse
    assert (4, 0) in LAYOUTS_F32 and (0, 4) in LAYOUTS_F32        # 4- but not 16-byte aligned, pointer or pitch


def test_geometry_keeps_its_guards():
    for host in _images():
        for lead, pitch in _layouts(host):
            r = Roi(host, lead, pitch, FILL_INPUT, device=None)
            g = r.geom
            assert g.first % 256 == lead and g.origin % 256 == 0
            assert g.first - GUARD_ROWS * pitch - GUARD_BYTES - lead >= 0                    # two rows above, and the lead in front of them
            assert g.total >= g.first + (g.rows + GUARD_ROWS) * pitch                        # two rows below
            assert pitch - g.width >= 2 * GUARD_BYTES + lead                                 # 16 bytes right of a row, 16 + lead left of the next
            assert np.array_equal(r.result(), host) and r.result().dtype == host.dtype
            outside = ~g.view_mask()
            assert outside.sum() == g.total - g.rows * g.width and (r.parent()[outside] == 0xFF).all()


def test_the_output_fill_depends_on_the_position():
    host = np.zeros((4, 8), np.uint8)
    a, b = Roi(host, 1, 64, FILL_OUTPUT, device=None, seed=1), Roi(host, 1, 64, FILL_OUTPUT, device=None, seed=1)
    assert np.array_equal(a.filled, b.filled)                                                # seeded
    out = a.filled[~a.geom.view_mask()]
    assert len(np.unique(out)) > 100                                                         # no constant store matches it
    assert not np.array_equal(a.filled, Roi(host, 1, 64, FILL_OUTPUT, device=None, seed=2).filled)


def test_an_f32_image_needs_aligned_pointer_and_pitch():
    host = np.zeros((2, 3), np.float32)
    for lead, pitch in ((2, 64), (0, 66), (1, 65)):
        with pytest.raises(AssertionError):
            Roi(host, lead, pitch, FILL_INPUT, device=None)
    Roi(np.zeros((2, 3), np.uint8), 1, 65, FILL_INPUT, device=None)                           # u8: any pointer and pitch
    with pytest.raises(AssertionError):
        Roi(host, 0, 3 * 4 + 16, FILL_INPUT, device=None)                                    # no room for the guards


def _plant(r, pos):
    r.base[pos] ^= 0x5A


@pytest.mark.parametrize("fill", [FILL_INPUT, FILL_OUTPUT])
def test_a_planted_byte_is_reported_where_it_lies(fill):
    for host in _images():
        for lead, pitch in _layouts(host):
            g = Roi(host, lead, pitch, fill, device=None).geom
            last = g.rows - 1
            spots = {
                "padding": (g.first + last * pitch + g.width, last, g.width),                # the byte right behind the last pixel
                "lead": (g.first - 1, 0, -1),                                                # the byte in front of the first pixel
                "guard rows above": (g.first - pitch + 2, -1, 2),
                "guard rows below": (g.first + g.rows * pitch + 1, g.rows, 1),
            }
            if g.rows > 1:
                spots["lead of a later row"] = (g.first + last * pitch - lead - GUARD_BYTES, last, -lead - GUARD_BYTES)
                spots["the padding's last byte"] = (g.first + pitch - lead - GUARD_BYTES - 1, 0, pitch - lead - GUARD_BYTES - 1)
            for region, (pos, row, byte) in spots.items():
                r = Roi(host, lead, pitch, fill, device=None)
                _plant(r, pos)
                with pytest.raises(AssertionError) as e:
                    r.result()
                name = "lead" if region.startswith("lead") else "padding" if "padding" in region else region
                assert f"1 bytes changed, first at (row {row}, byte {byte}: {name})" in str(e.value), (region, str(e.value))
                with pytest.raises(AssertionError):
                    r.assert_unchanged()
            # inside the view: nothing to say for an output, a modified input for assert_unchanged
            r = Roi(host, lead, pitch, fill, device=None)
            _plant(r, g.first + last * pitch + g.width - 1)
            got = r.result()
            assert (got != host).sum() == 1
            with pytest.raises(AssertionError) as e:
                r.assert_unchanged()
            assert f"an input was modified: 1 bytes changed, first at (row {last}, byte {g.width - 1}: view)" in str(e.value)
            # a clean parent passes both
            r = Roi(host, lead, pitch, fill, device=None)
            r.assert_unchanged()
            assert np.array_equal(r.result(), host)


def test_several_stray_bytes_are_counted_and_the_first_few_listed():
    host = np.zeros((6, 5), np.uint8)
    r = Roi(host, 3, 64, FILL_OUTPUT, device=None)
    g = r.geom
    for row in range(6):
        _plant(r, g.first + row * 64 + 5)
        _plant(r, g.first + row * 64 + 6)
    with pytest.raises(AssertionError) as e:
        r.result()
    msg = str(e.value)
    assert "12 bytes changed" in msg and "(row 0, byte 5: padding), (row 0, byte 6: padding), (row 1, byte 5: padding)" in msg
    assert msg.count("(row") == 6


def test_covering_keeps_every_pair():
    for counts in ((7, 7, 7), (7, 7, 7, 7), (7, 7), (7,), (7, 5, 7), (2, 7, 3, 7)):
        rows = covering(*counts)
        assert len(rows) <= max(49, counts[0] * (counts[1] if len(counts) > 1 else 1))
        for a in range(len(counts)):
            assert {t[a] for t in rows} == set(range(counts[a]))
            for b in range(a + 1, len(counts)):
                assert {(t[a], t[b]) for t in rows} == {(i, j) for i in range(counts[a]) for j in range(counts[b])}
