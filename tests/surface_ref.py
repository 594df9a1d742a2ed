"""rtdd_fill_surface restated (include/rtdd.h, "the wand that follows the depth map"): test infrastructure.

A surface wand is the 12-tuple (x, y, step, below, above, flags, ax0, ay0, ax1, ay1, label0, label1) of rtdd_surface_wand.  Three routes to
the covered set: `covered_queue` is the header's rule as it stands -- the clamped depth, the band and every difference in f32 numpy scalars,
the component by an explicit queue (the yardstick); `covered_graph` is scipy.sparse.csgraph.connected_components over the list of links;
`covered_tiled` restates the kernels' schedule -- the three uint64 planes H, V and reach, the link carry fill, 64 x 64 blocks with halos,
Jacobi passes (every block reads the state the pass BEFORE left) to the fixpoint -- and also returns the number of passes, the last,
changeless one included: an upper bound on what the device needs.  tests/test_fill_surface_cpu.py pins the three against each other.  The
writes are polygon_ref's; the shapes that make the schedule work are wand_ref's."""
from collections import deque

import numpy as np

import polygon_ref as pr
import wand_ref as wr
from wand_ref import BLOCK, STROKE_ERASE, comb, comb_seed, info_of, spiral  # noqa: F401

SURFACE_GLOBAL = 1
f32 = np.float32
_ONE, _SHIFT63 = np.uint64(1), np.uint64(63)


def constant(x, y, step, label, below=255, above=255, flags=0):
    return (x, y, step, below, above, flags, 0, 0, 0, 0, label, label)


def erase(x, y, step, below=255, above=255, flags=0):
    return (x, y, step, below, above, flags, 0, 0, 0, 0, STROKE_ERASE, STROKE_ERASE)


def clamped(depth):
    """d' = d > 0 ? fminf(d, 255) : +0 -- a NaN, -0 and every negative are +0, +inf is 255"""
    d = np.asarray(depth, f32)
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, np.fmin(d, f32(255)), f32(0)).astype(f32)


def band(dc, wand):
    """(lo, hi) as f32 scalars, each one f32 operation"""
    x, y = int(wand[0]), int(wand[1])
    ds = f32(dc[y, x])
    return f32(ds - f32(wand[3])), f32(ds + f32(wand[4]))


def admissible(dc, wand):
    lo, hi = band(dc, wand)
    return (lo <= dc) & (dc <= hi)


def links(dc, wand):
    """(H, V) as bool [rows, cols]: H[y, x] the link (x, y) - (x + 1, y), V[y, x] the link (x, y) - (x, y + 1); the last column of H and
    the last row of V are False."""
    a = admissible(dc, wand)
    step = f32(wand[2])
    H, V = np.zeros(dc.shape, bool), np.zeros(dc.shape, bool)
    H[:, :-1] = a[:, :-1] & a[:, 1:] & (np.abs(dc[:, :-1] - dc[:, 1:]) <= step)          # (f32 arrays: one f32 subtraction)
    V[:-1, :] = a[:-1, :] & a[1:, :] & (np.abs(dc[:-1, :] - dc[1:, :]) <= step)
    return H, V


def covered_queue(depth, wand):
    x, y = int(wand[0]), int(wand[1])
    step, flags = f32(wand[2]), int(wand[5])
    dc = clamped(depth)
    rows, cols = dc.shape
    lo, hi = band(dc, wand)
    adm = lambda v: bool(lo <= v) and bool(v <= hi)
    if flags & SURFACE_GLOBAL:
        return np.array([[adm(dc[j, i]) for i in range(cols)] for j in range(rows)], bool).reshape(rows, cols)
    out = np.zeros((rows, cols), bool)
    out[y, x] = True
    todo = deque([(x, y)])
    while todo:
        px, py = todo.popleft()
        p = dc[py, px]
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            qx, qy = px + dx, py + dy
            if not (0 <= qx < cols and 0 <= qy < rows) or out[qy, qx]:
                continue
            q = dc[qy, qx]
            if adm(p) and adm(q) and bool(np.abs(f32(p - q)) <= step):
                out[qy, qx] = True
                todo.append((qx, qy))
    return out


def covered_graph(depth, wand):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    dc = clamped(depth)
    rows, cols = dc.shape
    if int(wand[5]) & SURFACE_GLOBAL:
        return admissible(dc, wand)
    H, V = links(dc, wand)
    idx = np.arange(rows * cols).reshape(rows, cols)
    a = np.concatenate((idx[H], idx[V]))
    b = np.concatenate((idx[H] + 1, idx[V] + cols))
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(rows * cols, rows * cols))
    _, lab = connected_components(g, directed=False)
    lab = lab.reshape(rows, cols)
    return lab == lab[int(wand[1]), int(wand[0])]


# ---- the kernels' schedule -------------------------------------------------------------------------------------------------------------
def fill_links_bits(h, r, bits):
    """The kernel's horizontal fill on words of `bits` bits (Python integers or int64 arrays): bit x of h links x to x + 1 (the top bit:
    the link into the next word, whose carry out is dropped, as a register drops it).  Towards higher bits r | ((h + (r & h)) ^ h);
    towards lower bits the same on the reversed words with the reversed links one further down."""
    m = (1 << bits) - 1

    def up(h_, r_):
        return r_ | (((h_ + (r_ & h_)) & m) ^ h_)

    r = up(h, r)
    return wr.brev_bits(up(wr.brev_bits(h, bits) >> 1, wr.brev_bits(r, bits)), bits)


def fill_links_naive(h, r, bits):
    """The same by iteration: a bit beside a reached bit is reached where the link between them is set, `bits` times over."""
    m = (1 << bits) - 1
    for _ in range(bits):
        r = (r | ((r & h) << 1) | ((r >> 1) & h)) & m
    return r


def _up64(h, r):
    return r | ((h + (r & h)) ^ h)                                    # (uint64 arrays: the sum wraps)


def fill_links64(h, r):
    return wr._brev64(_up64(wr._brev64(h) >> _ONE, wr._brev64(_up64(h, r))))


def _block_pass(H, V, old, new, bx, y0):
    """One wave's work on planes padded by a zero word all round and to whole blocks (block (bx, y0) lies at [y0 + 1 : y0 + 65, bx + 1]):
    the block to its own fixpoint in "registers" against the halo of `old`, read once, every halo bit under its link."""
    rs = slice(y0 + 1, y0 + BLOCK + 1)
    h, v, r0 = H[rs, bx + 1], V[rs, bx + 1], old[rs, bx + 1]
    side = ((old[rs, bx] & H[rs, bx]) >> _SHIFT63) | ((old[rs, bx + 2] << _SHIFT63) & h)
    above = old[y0, bx + 1] & V[y0, bx + 1]
    below = old[y0 + BLOCK + 1, bx + 1] & v[-1]
    if not (r0.any() or side.any() or above or below):
        return False
    r = r0.copy()
    while True:
        rv = r & v
        up = np.concatenate(([above], rv[:-1]))
        dn = np.concatenate((r[1:], [old[y0 + BLOCK + 1, bx + 1]])) & v
        nxt = fill_links64(h, r | side | up | dn)
        if np.array_equal(nxt, r):
            break
        r = nxt
    if np.array_equal(r, r0):
        return False
    new[rs, bx + 1] = r
    return True


def covered_tiled(depth, wand):
    """(covered mask, passes): the three planes, and Jacobi passes over all blocks until one changes nothing (that one is counted)."""
    x, y = int(wand[0]), int(wand[1])
    dc = clamped(depth)
    rows, cols = dc.shape
    if int(wand[5]) & SURFACE_GLOBAL:
        return admissible(dc, wand), 0
    Hm, Vm = links(dc, wand)
    assert not Hm[:, -1].any() and not Vm[-1, :].any()
    hw, vw = wr.pack_words(Hm), wr.pack_words(Vm)
    W, R = hw.shape[1], (rows + BLOCK - 1) // BLOCK * BLOCK
    H, V = np.zeros((R + 2, W + 2), np.uint64), np.zeros((R + 2, W + 2), np.uint64)
    H[1:rows + 1, 1:W + 1] = hw
    V[1:rows + 1, 1:W + 1] = vw
    reach = np.zeros_like(H)
    reach[y + 1, (x >> 6) + 1] = _ONE << np.uint64(x & 63)
    passes = 0
    while True:
        passes += 1
        new = reach.copy()
        changed = [_block_pass(H, V, reach, new, bx, y0) for y0 in range(0, R, BLOCK) for bx in range(W)]
        reach = new
        if not any(changed):
            return wr.unpack_words(reach[1:rows + 1, 1:W + 1], cols), passes


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
INSIDE, OUTSIDE = f32(60), f32(200)


def from_mask(mask):
    """A two-level depth map: INSIDE where the mask is set, OUTSIDE elsewhere: with a step below 140 a seed inside selects the mask's
    4-connected component."""
    return np.where(mask, INSIDE, OUTSIDE).astype(f32)


def field(rng, rows, cols):
    """A random depth map of four levels 2.5 apart, half of it in 3 x 3 patches and half per pixel, each pixel lifted by 0 .. 1 in
    quarters: every value is exact in f32, and the STEPS below separate the levels differently."""
    patches = rng.integers(0, 4, ((rows + 2) // 3, (cols + 2) // 3)).repeat(3, 0).repeat(3, 1)[:rows, :cols]
    lvl = np.where(rng.random((rows, cols)) < 0.5, patches, rng.integers(0, 4, (rows, cols)))
    return (f32(100) + f32(2.5) * lvl + rng.integers(0, 5, (rows, cols)) * f32(0.25)).astype(f32)


STEPS = (7.5, 0, 1, 2.5, 3.5, 5)
BANDS = ((255, 255), (3, 3), (255, 2), (0, 255), (6, 6), (255, 255))


SEEDS_67x45 = [(0, 0), (44, 0), (0, 66), (44, 66), (20, 63), (21, 64), (44, 30)]


def random_cases(seed, flags, rows=67, cols=45):
    """The GPU test's draw order: the field, then the seed when it is drawn."""
    rng = np.random.default_rng(seed)
    for i, s in enumerate(SEEDS_67x45 + [None] * 5):
        depth = field(rng, rows, cols)
        x, y = s if s is not None else (int(rng.integers(0, cols)), int(rng.integers(0, rows)))
        below, above = BANDS[(i // 2) % 6]
        yield i, depth, (x, y, STEPS[i % 6], below, above, flags)


def special_field(rng, rows, cols):
    """field with NaN, -0, -5, 0, 1e-40, 300, +inf, 255 and -inf sprinkled in, a run of NaN / -0 / -5 / 0 / -inf among them"""
    depth = field(rng, rows, cols)
    values = np.array([np.nan, -0.0, -5, 0, 1e-40, 300, np.inf, 255, -np.inf], f32)
    where = rng.random((rows, cols)) < 0.3
    depth[where] = values[rng.integers(0, len(values), int(where.sum()))]
    depth[5, 3:8] = [np.nan, -0.0, -5, 0, -np.inf]
    depth[6, 5] = f32(1e-40)                                          # a denormal is not +0
    return depth


def kinds(x, y, step, below, above, flags, rows, cols):
    """a constant label, a ramp across the image, an eraser"""
    return (constant(x, y, step, 77, below, above, flags), (x, y, step, below, above, flags, 3, -4, cols - 5, rows + 6, 5, 250),
            erase(x, y, step, below, above, flags))


# ---- the call --------------------------------------------------------------------------------------------------------------------------
def fill_surface(wand, edited, scribble, depth, original=None, covered=covered_queue):
    """rtdd_fill_surface in place on edited [rows, cols, 3] and scribble [rows, cols]; returns info_of the covered set."""
    m = covered(depth, wand)
    if isinstance(m, tuple):
        m = m[0]
    pr._write((0,) + tuple(wand[6:]), edited, scribble, original, 0, 0, m)
    return info_of(m)
