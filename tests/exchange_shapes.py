"""Shapes for the persistent sweep's exchange record (csrc/sweep_blocked.hip: `xrec`), derived from tests/tile_geometry.py -- NOT read
from the library.  Imports without a GPU: tests/test_exchange_shapes_cpu.py pins what the shapes cover, tests/test_gpu_exchange_record.py
runs the kernels on them.

At every halo exchange a thread reads back one record, built once per launch: where its 4-pixel group lies in a plane (a 32-bit byte
offset), which of its G rows it stores (its tile's centre, within two halo widths of the centre's edge) and loads (halo inside the
image), and whether the group straddles the image's right edge (`cols` is no multiple of 4 and the group holds column cols - 1): only
a wave with such a group takes the path that zeroes the pixels beyond the edge.  `thread_record` restates those rules."""
from collections import namedtuple

import tile_geometry as tg

TILES = (4, 6, 9)                        # LX 32 / G 3, LX 16 / G 3, LX 16 / G 1
DEPTHS = (4, 8)

Case = namedtuple("Case", "tile T rows cols n tag")


def shapes(tile, T):
    """A 3 x 3 grid of tiles with a ragged last tile row (1 .. hy - 1 rows), in two widths: 2*TW + hx + 1 -- cols % 4 == 1, and the last
    tile column's extended tile crosses `cols`: the select path -- and 3*TW -- cols % 4 == 0: no group straddles, no select."""
    g = tg.geometry(tile, T)
    rows = 2 * g.TH + g.hy // 2 + 1
    return [tg.Shape(rows, 2 * g.TW + g.hx + 1, "straddle"), tg.Shape(rows, 3 * g.TW, "multiple-of-4")]


def cases(tile):
    """Depths 4 and 8, both widths, sweep counts 2*T + 3 (3 blocks, a tail of 3 sweeps, the result in the spare plane pair) and 3*T
    (3 blocks, no tail): between them both parities of the exchange buffers are written and read."""
    return [Case(tile, T, s.rows, s.cols, n, s.tag) for T in DEPTHS for s in shapes(tile, T) for n in (2 * T + 3, 3 * T)]


def thread_record(tile, T, rows, cols, by, bx, lx, tr):
    """(store rows, load rows, pixels of the group left of `cols`, straddles) of thread (lane lx of thread row tr) of tile (by, bx)."""
    LX, NT, G = tg.TILES[tile]
    g = tg.geometry(tile, T)
    x0, y0 = bx * g.TW - g.hx + 4 * lx, by * g.TH - g.hy + tr * G
    colok = 0 <= x0 < cols
    xin = colok and g.hx <= 4 * lx < g.EW - g.hx
    store, load = [], []
    for r in range(G):
        y, ty = y0 + r, tr * G + r
        central = xin and g.hy <= ty < g.EH - g.hy
        band = ty < 2 * g.hy or ty >= g.EH - 2 * g.hy or 4 * lx < 2 * g.hx or 4 * lx >= g.EW - 2 * g.hx
        ok = colok and 0 <= y < rows
        if central and y < rows and band:
            store.append(r)
        if ok and not central:
            load.append(r)
    nv = min(max(cols - x0, 0), 4)
    return store, load, nv, colok and nv < 4


def straddling_loads(tile, T, rows, cols, by, bx):
    """How many threads of tile (by, bx) LOAD a row of a group that straddles `cols`."""
    LX, NT, G = tg.TILES[tile]
    n = 0
    for tr in range(NT // LX):
        for lx in range(LX):
            _, load, _, straddles = thread_record(tile, T, rows, cols, by, bx, lx, tr)
            n += bool(load and straddles)
    return n


def interior_tiles(tile, T, rows, cols):
    """Tiles with all 8 neighbours in the grid: they trade strips on every side."""
    gy, gx = tg.grid(tile, T, rows, cols)
    return [(by, bx) for by in range(1, gy - 1) for bx in range(1, gx - 1)]
