"""The blocked sweeps' tile geometry, restated from the tile table (csrc/sweep_blocked.hip: kTiles, launch_sweeps_blocked_impl and the
kernels' own `tile_inside`) -- NOT read from the library -- and the boundary shapes that follow from it for one (tile, depth).
Imports without a GPU: tests/test_tile_geometry_cpu.py pins it, tests/test_gpu_tile_geometry.py runs the kernels on its shapes.

A tile of id t is EW = 4*LX pixels wide and EH = NT/LX*G rows high; with T sweeps per launch (or per halo exchange) its halo is
hx = T rounded up to 4 columns and hy = T rows, and what it writes back is its centre, TW = EW - 2*hx by TH = EH - 2*hy."""
from collections import namedtuple

# id -> (LX lanes per tile row, NT threads, G rows per thread): RTDD_ALL_TILES (1-13) and kTiles' column-layout tiles (14-16)
TILES = {1: (16, 256, 4), 2: (32, 512, 4), 3: (32, 1024, 4), 4: (32, 1024, 3), 5: (32, 512, 3), 6: (16, 512, 3), 7: (16, 256, 3),
         8: (32, 1024, 2), 9: (16, 1024, 1), 10: (16, 512, 2), 11: (32, 1024, 1), 12: (32, 768, 4), 13: (32, 512, 6),
         14: (16, 1024, 1), 15: (16, 512, 1), 16: (16, 768, 1)}
ROW_TILES = tuple(range(1, 14))          # k_sweep_blocked: the only ones with a persistent mode
ALL_TILES = tuple(range(1, 17))
MAX_DEPTH = 28
NUM_CUS = 256                            # MI355X; never the limit at these sizes

Geometry = namedtuple("Geometry", "EW EH T hx hy TW TH")
Shape = namedtuple("Shape", "rows cols tag")


def _ceil(a, b):
    return -(-a // b)


def geometry(tile, T):
    """EW, EH, the depth the host's clamp leaves (at most 28, and a written-back region of at least 8 x 8), hx, hy, TW, TH."""
    LX, NT, G = TILES[tile]
    EW, EH = 4 * LX, NT // LX * G
    T = min(T, MAX_DEPTH)
    while T > 1 and (EW - 2 * ((T + 3) // 4 * 4) < 8 or EH - 2 * T < 8):
        T -= 1
    hx, hy = (T + 3) // 4 * 4, T
    return Geometry(EW, EH, T, hx, hy, EW - 2 * hx, EH - 2 * hy)


def largest_unclamped_depth(tile):
    return max(T for T in range(1, MAX_DEPTH + 1) if geometry(tile, T).T == T)


def is_single(tile, rows, cols):
    """The whole level fits the extended tile: one workgroup, no halo, every sweep in one launch."""
    g = geometry(tile, 1)
    return cols <= g.EW and rows <= g.EH


def grid(tile, T, rows, cols):
    """(tile rows, tile columns) of a launch whose blocks are all T sweeps long."""
    if is_single(tile, rows, cols):
        return 1, 1
    g = geometry(tile, T)
    return _ceil(rows, g.TH), _ceil(cols, g.TW)


def tile_inside(tile, T, rows, cols, by, bx):
    """The kernels' wave-uniform fast path: the whole extended tile, its pixels' right and lower neighbours and the row above it are inside the image."""
    g = geometry(tile, T)
    tx0, ty0 = bx * g.TW - g.hx, by * g.TH - g.hy
    return tx0 >= 0 and tx0 + g.EW < cols and ty0 >= 1 and ty0 + g.EH < rows


def inside_tiles(tile, T, rows, cols):
    gy, gx = grid(tile, T, rows, cols)
    if is_single(tile, rows, cols):
        return []
    return [(by, bx) for by in range(gy) for bx in range(gx) if tile_inside(tile, T, rows, cols, by, bx)]


def persistent_expected(tile, T, rows, cols, n, num_cus=NUM_CUS, images=1):
    """launch_sweeps_blocked_impl's conditions for ONE launch with halo exchanges (RTDD_OPT_PERSISTENT = 1 and the kernel's occupancy
    granted): not a single tile, a row-layout tile, an even depth, more than one block, the halo inside the 8 neighbours' centres,
    every workgroup resident."""
    if is_single(tile, rows, cols) or tile >= 14:
        return False
    g = geometry(tile, T)
    gy, gx = grid(tile, T, rows, cols)
    return g.T % 2 == 0 and n > g.T and g.hx <= g.TW and g.hy <= g.TH and gy * gx * images <= num_cus


def launches_expected(tile, T, rows, cols, n, persistent_option, images=1):
    if is_single(tile, rows, cols):
        return 1
    if persistent_option and persistent_expected(tile, T, rows, cols, n, images=images):
        return 1
    return _ceil(n, geometry(tile, T).T)


def last_block_expected(tile, T, rows, cols, n, persistent_option, images=1):
    """rtdd_solve_info.temporal_depth: the sweeps of the LAST launch, or the sweeps between two exchanges of a persistent one."""
    if is_single(tile, rows, cols):
        return n
    T = geometry(tile, T).T
    if persistent_option and persistent_expected(tile, T, rows, cols, n, images=images):
        return T
    return n - (_ceil(n, T) - 1) * T


def _edges(tile, T):
    """The row values R and column values C of shapes(), and the index (ky, kx) of the first tile row / column that can be inside.

    kx = ceil(hx / TW) and ky = ceil((hy + 1) / TH): tile column kx is the first with tx0 >= 0, tile row ky the first with ty0 >= 1
    (`tile_inside` wants the row ABOVE the tile inside the image too, so with hy == TH the first candidate is row 2).  Wherever the halo
    fits inside a neighbour's centre with a row to spare both are 1 and the lists are 2*TW, 2*TW + 1, 2*TW + hx - 1, 2*TW + hx,
    2*TW + hx + 1, 3*TW - 1, 3*TW: tile column 1 ends at tx0 + EW = 2*TW + hx, the last width at which it is not inside.  Deeper halos
    (the column tiles at depth 28 have 8 x 8 centres under a 28-pixel halo) move the same seven values out to tile column kx."""
    g = geometry(tile, T)
    kx, ky = _ceil(g.hx, g.TW), _ceil(g.hy + 1, g.TH)

    def seven(k, t, h):
        b = (k + 1) * t
        return [b, b + 1, b + h - 1, b + h, b + h + 1, (k + 2) * t - 1, (k + 2) * t]
    return seven(ky, g.TH, g.hy), seven(kx, g.TW, g.hx), ky, kx


def _whole_rounds_grid(tile, T):
    """The smallest grid of at least (ky + 3) x (kx + 3) tiles whose tile count is a multiple of 8 and whose one-pixel-corner shape is not single."""
    g = geometry(tile, T)
    _, _, ky, kx = _edges(tile, T)
    best = None
    for gy in range(ky + 3, ky + 12):
        for gx in range(kx + 3, kx + 12):
            if gy * gx % 8 == 0 and not is_single(tile, (gy - 1) * g.TH + 1, (gx - 1) * g.TW + 1) and (best is None or gy * gx < best[0] * best[1]):
                best = (gy, gx)
    return best


def shapes(tile, T):
    """The boundary shapes of (tile, T), each with the construction it comes from; no duplicates, no single-tile shape."""
    g = geometry(tile, T)
    R, C, ky, kx = _edges(tile, T)
    out = [(R[i], C[i], "diagonal") for i in range(7)] + [(R[6 - i], C[i], "anti-diagonal") for i in range(7)]
    # one boundary of `tile_inside` alone, the other dimension well inside (on the two diagonals rows and columns cross their
    # boundaries together, or one of them is short of it)
    out += [(R[4], C[3], "cross"), (R[3], C[4], "cross")]
    out += [(1, C[1], "thin"), (g.TH, C[4], "thin"), (R[1], g.EW + 1, "thin"), (R[4], g.TW, "thin")]
    # a tile count that is a multiple of 8 (the XCD placement's workgroups all have a tile), a corner tile with a one-pixel centre:
    # (3*TH + 1, 3*TW + 1), 4 x 4 tiles, wherever ky = kx = 1
    gy8, gx8 = _whole_rounds_grid(tile, T)
    out.append(((gy8 - 1) * g.TH + 1, (gx8 - 1) * g.TW + 1, "whole-xcd-rounds"))
    seen, res = set(), []
    for rows, cols, tag in out:
        if (rows, cols) in seen or is_single(tile, rows, cols):
            continue
        seen.add((rows, cols))
        res.append(Shape(rows, cols, tag))
    return res


def max_grid(tile, T):
    """No shape of shapes() has more tile rows / columns than this: 4 x 4 wherever ky = kx = 1."""
    g = geometry(tile, T)
    _, _, ky, kx = _edges(tile, T)
    gy8, gx8 = _whole_rounds_grid(tile, T)
    return max(gy8, _ceil((ky + 1) * g.TH + g.hy + 1, g.TH)), max(gx8, _ceil((kx + 1) * g.TW + g.hx + 1, g.TW))


def classes(tile, T, rows, cols):
    """The geometry classes a shape serves for (tile, T), derived from the restated geometry alone."""
    g = geometry(tile, T)
    gy, gx = grid(tile, T, rows, cols)
    R, C, ky, kx = _edges(tile, T)
    last_w, last_h = cols - (gx - 1) * g.TW, rows - (gy - 1) * g.TH        # the last tile column's / row's centre
    out = set()
    ragged_w, ragged_h = gx > 1 and 1 <= last_w < g.hx, gy > 1 and 1 <= last_h < g.hy
    if ragged_w: out.add("ragged-width")
    if ragged_h: out.add("ragged-height")
    if ragged_w and ragged_h: out.add("ragged-both")
    if gx > 1 and last_w == 1 and gy > 1 and last_h == 1: out.add("one-pixel-corner")
    if inside_tiles(tile, T, rows, cols): out.add("inside")
    # one short of a boundary of tile (ky, kx)'s `tile_inside`, the other dimension satisfied
    if cols == C[3] and rows > R[3] and not tile_inside(tile, T, rows, cols, ky, kx): out.add("columns-one-short-of-inside")
    if rows == R[3] and cols > C[3] and not tile_inside(tile, T, rows, cols, ky, kx): out.add("rows-one-short-of-inside")
    if cols == C[4] and rows > R[3] and tile_inside(tile, T, rows, cols, ky, kx): out.add("columns-just-inside")
    if rows == R[4] and cols > C[3] and tile_inside(tile, T, rows, cols, ky, kx): out.add("rows-just-inside")
    if gy == 1 and gx > 1: out.add("thin-row")
    if gx == 1 and gy > 1: out.add("thin-column")
    out.add("tiles-multiple-of-8" if gy * gx % 8 == 0 else "tiles-not-multiple-of-8")
    return out


REQUIRED_CLASSES = ("ragged-width", "inside", "columns-one-short-of-inside", "rows-one-short-of-inside", "columns-just-inside", "rows-just-inside",
                    "thin-row", "thin-column", "one-pixel-corner", "tiles-multiple-of-8", "tiles-not-multiple-of-8")
DEEP_ONLY_CLASSES = ("ragged-height", "ragged-both")      # a last tile row of 1 .. hy-1 rows needs hy >= 2


# ---- the cases of tests/test_gpu_tile_geometry.py --------------------------------------------------------------------------------
PERSISTENT_DEPTHS = (2, 4, 8, 12, 16, 20)


def launch_per_block_depths(tile):
    """1, 5, 8, 28 and the largest depth the clamp leaves alone, as ASKED of the library: where the clamp lowers 28 to that depth it is 28
    that is asked for, so that the host's clamp runs and the helper has to predict it."""
    out = []
    for T in (1, 5, 8, 28, largest_unclamped_depth(tile)):
        if geometry(tile, T).T not in [geometry(tile, t).T for t in out]:
            out.append(T)
    return out


def persistent_depths(tile):
    """Every depth of 2, 4, 8, 12, 16, 20 at which the tile's halo fits its neighbours' centres (and the clamp leaves the depth alone)."""
    out = []
    for T in PERSISTENT_DEPTHS:
        g = geometry(tile, T)
        if g.T == T and g.hx <= g.TW and g.hy <= g.TH:
            out.append(T)
    return out


def launch_per_block_cases(tile):
    """(asked depth, Shape, n) with n round-robin over T - 1 (when >= 1), T, T + 1 and 2*T + 3 of the clamped depth T."""
    out, turn = [], 0
    for asked in launch_per_block_depths(tile):
        T = geometry(tile, asked).T
        ns = [n for n in (T - 1, T, T + 1, 2 * T + 3) if n >= 1]
        for s in shapes(tile, asked):
            out.append((asked, s, ns[turn % len(ns)]))
            turn += 1
        turn += 1                                # (so that a shape does not meet the same kind of n at every depth)
    return out


def persistent_cases(tile):
    """(depth, Shape, n) with n round-robin over T + 1, 2*T, 2*T + 3, 3*T and 4*T + 1: 2, 2, 3, 3 and 5 blocks, so both parities of
    the plane pair that ends up holding the result, and tail blocks of 1 and 3 sweeps."""
    out, turn = [], 0
    for T in persistent_depths(tile):
        ns = (T + 1, 2 * T, 2 * T + 3, 3 * T, 4 * T + 1)
        for s in shapes(tile, T):
            out.append((T, s, ns[turn % len(ns)]))
            turn += 1
        turn += 1
    return out


BATCH_TILES = (4, 6, 9)
BATCH_DEPTH = 8
BATCH_IMAGES = 3


def batch_shapes(tile):
    """One shape whose last tile row AND column are ragged, and the whole-XCD-rounds shape (4 x 4 tiles at depth 8)."""
    ss = shapes(tile, BATCH_DEPTH)
    both = next(s for s in ss if "ragged-both" in classes(tile, BATCH_DEPTH, s.rows, s.cols))
    whole = next(s for s in ss if s.tag == "whole-xcd-rounds")
    return [both, whole]
