"""What tests/exchange_shapes.py's shapes cover, from the restated geometry alone (no GPU, no library): every case runs persistently
on a 3 x 3 grid with a ragged last tile row; the `straddle` width has cols % 4 == 1 and at least one tile that LOADS a group lying
across the image's right edge (the exchange's select path) next to an interior tile that loads none (the common path in the same
launch); the `multiple-of-4` width has no straddling group anywhere."""
import pytest

import exchange_shapes as xs
import tile_geometry as tg


@pytest.mark.parametrize("tile", xs.TILES)
def test_the_shapes_reach_both_paths_of_the_exchange(tile):
    seen = set()
    for c in xs.cases(tile):
        g = tg.geometry(c.tile, c.T)
        assert g.T == c.T and tg.grid(c.tile, c.T, c.rows, c.cols) == (3, 3), c
        assert tg.persistent_expected(c.tile, c.T, c.rows, c.cols, c.n) and tg.launches_expected(c.tile, c.T, c.rows, c.cols, c.n, 1) == 1, c
        assert "ragged-height" in tg.classes(c.tile, c.T, c.rows, c.cols), c
        tiles = [(by, bx) for by in range(3) for bx in range(3)]
        straddling = {t: xs.straddling_loads(c.tile, c.T, c.rows, c.cols, *t) for t in tiles}
        interior = xs.interior_tiles(c.tile, c.T, c.rows, c.cols)
        assert interior == [(1, 1)]
        if c.tag == "straddle":
            assert c.cols % 4 == 1 and c.cols == 2 * g.TW + g.hx + 1
            assert any(n > 0 for n in straddling.values()), c                # some tile loads a group across the edge ...
            assert all(bx == 2 for (by, bx), n in straddling.items() if n), straddling      # ... in the last tile column only
            assert straddling[(1, 1)] == 0                                    # the interior tile takes the path without the select
        else:
            assert c.cols % 4 == 0 and c.cols == 3 * g.TW
            assert not any(straddling.values()), straddling
        # the interior tile stores and loads on all four sides
        LX, NT, G = tg.TILES[c.tile]
        recs = [xs.thread_record(c.tile, c.T, c.rows, c.cols, 1, 1, lx, tr) for tr in range(NT // LX) for lx in range(LX)]
        assert any(r[0] for r in recs) and any(r[1] for r in recs) and not any(set(r[0]) & set(r[1]) for r in recs)
        seen.add((c.T, c.tag, (c.n + c.T - 1) // c.T, c.n % c.T))
    # both depths x both widths, 3 blocks each, with a tail of 3 sweeps and without one
    assert seen == {(T, tag, 3, tail) for T in xs.DEPTHS for tag in ("straddle", "multiple-of-4") for tail in (0, 3)}
