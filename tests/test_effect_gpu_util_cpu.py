"""tests/effect_gpu.py's own helpers on the CPU: an assertion helper that passed vacuously would hide failures in every file that uses it."""
import numpy as np
import pytest

from effect_gpu import FILL, assert_padding_untouched, assert_same_image, padded_artistic, read_pnm, tile_mirrored, write_pnm


def test_assert_same_image_counts_the_differing_pixels():
    a = np.arange(45, dtype=np.uint8).reshape(3, 5, 3)
    assert_same_image(a, a.copy(), "equal")
    b = a.copy()
    b[1, 3, 2] ^= 1                                         # one channel of one pixel
    with pytest.raises(AssertionError, match="1 of 15 pixels"):
        assert_same_image(b, a, "one channel")
    with pytest.raises(AssertionError, match="shapes"):
        assert_same_image(a[:, :4], a, "another shape")


def test_tile_mirrored():
    a = np.array([[0, 1, 2], [3, 4, 5]], np.float32)
    want = np.array([[0, 1, 2, 2, 1, 0, 0],
                     [3, 4, 5, 5, 4, 3, 3],
                     [3, 4, 5, 5, 4, 3, 3],
                     [0, 1, 2, 2, 1, 0, 0],
                     [0, 1, 2, 2, 1, 0, 0]], np.float32)
    got = tile_mirrored(a, 5, 7)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)


def test_pnm_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for name, a in (("c.ppm", rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)), ("g.pgm", rng.integers(0, 256, (4, 5), dtype=np.uint8))):
        write_pnm(tmp_path / name, a)
        back = read_pnm(tmp_path / name)
        assert back.shape == a.shape and np.array_equal(back, a)
    assert (tmp_path / "c.ppm").read_bytes().startswith(b"P6\n5 4\n255\n") and (tmp_path / "g.pgm").read_bytes().startswith(b"P5\n5 4\n255\n")


def test_padding_check_sees_one_byte():
    rows, cols, pitch = 3, 5, 5 * 3 + 13
    base, art = padded_artistic(rows, cols, pitch, device="cpu")
    assert base.shape == (rows, pitch) and art.shape == (rows, cols, 3) and bool((base == FILL).all())
    assert_padding_untouched(base, cols)
    art[2, 4, 2] = FILL ^ 0xFF                              # the last byte of the image: a view of base, and not padding
    assert int(base[2, cols * 3 - 1]) == FILL ^ 0xFF
    assert_padding_untouched(base, cols)
    base[1, cols * 3] = 0                                   # the first padding byte of a row
    with pytest.raises(AssertionError, match="padding bytes written"):
        assert_padding_untouched(base, cols)
    base[1, cols * 3] = FILL
    base[2, pitch - 1] = FILL + 1                           # the last one of the buffer
    with pytest.raises(AssertionError, match="padding bytes written"):
        assert_padding_untouched(base, cols)
