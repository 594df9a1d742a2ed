"""rtdd_fill_similar restated (include/rtdd.h, "the magic wand"): test infrastructure.

A wand is the 10-tuple (x, y, tolerance, flags, ax0, ay0, ax1, ay1, label0, label1) of rtdd_wand.  Three routes to the covered set:
`covered_queue` is the header's rule as it stands -- eligibility in numpy, the component by an explicit queue in Python integers (the
yardstick); `covered_label` is scipy.ndimage.label with the cross or the 3 x 3 structure; `covered_tiled` restates the kernels' schedule --
uint64 words, the carry fill, 64 x 64 blocks with halos, Jacobi passes (every block reads the state the pass BEFORE left) to the fixpoint --
and also returns the number of passes, the last, changeless one included: an upper bound on what the device needs, since a block there may
also see what a neighbour wrote in the same pass.  tests/test_fill_similar_cpu.py pins the three against each other.  The writes are
polygon_ref's (the label rule is ramp_ref's)."""
from collections import deque

import numpy as np

import polygon_ref as pr

WAND_CONNECT_8, WAND_GLOBAL = 1, 2
STROKE_ERASE = -1
BLOCK = 64
FULL = (1 << 64) - 1


def constant(x, y, tolerance, label, flags=0):
    return (x, y, tolerance, flags, 0, 0, 0, 0, label, label)


def erase(x, y, tolerance, flags=0):
    return (x, y, tolerance, flags, 0, 0, 0, 0, STROKE_ERASE, STROKE_ERASE)


def eligible(original, x, y, tolerance):
    """The eligibility mask: Chebyshev distance of every pixel's (B, G, R) to the seed's, at most `tolerance`."""
    o = original.astype(np.int64)
    return np.abs(o - o[y, x]).max(-1) <= tolerance


def _steps(flags):
    four = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    return four + [(-1, -1), (1, -1), (-1, 1), (1, 1)] if flags & WAND_CONNECT_8 else four


def covered_queue(original, wand):
    x, y, tolerance, flags = (int(v) for v in wand[:4])
    rows, cols = original.shape[:2]
    e = eligible(original, x, y, tolerance)
    if flags & WAND_GLOBAL:
        return e
    out = np.zeros((rows, cols), bool)
    out[y, x] = True
    todo = deque([(x, y)])
    steps = _steps(flags)
    while todo:
        px, py = todo.popleft()
        for dx, dy in steps:
            qx, qy = px + dx, py + dy
            if 0 <= qx < cols and 0 <= qy < rows and e[qy, qx] and not out[qy, qx]:
                out[qy, qx] = True
                todo.append((qx, qy))
    return out


def covered_label(original, wand):
    from scipy import ndimage
    x, y, tolerance, flags = (int(v) for v in wand[:4])
    e = eligible(original, x, y, tolerance)
    if flags & WAND_GLOBAL:
        return e
    lab, _ = ndimage.label(e, structure=np.ones((3, 3), int) if flags & WAND_CONNECT_8 else ndimage.generate_binary_structure(2, 1))
    return lab == lab[y, x]


# ---- the kernels' schedule -------------------------------------------------------------------------------------------------------------
def brev_bits(v, bits):
    """The low `bits` bits of v in reverse order (v a Python integer or an integer array)."""
    out = v * 0
    for i in range(bits):
        out = out | (((v >> i) & 1) << (bits - 1 - i))
    return out


def fill_row_bits(e, r, bits):
    """The kernel's horizontal fill on words of `bits` bits (Python integers or int64 arrays; the carry out of the top bit is dropped, as
    a register drops it): every bit of e joined to a bit of r (r a subset of e) through bits of e.  Towards higher bits adding r to e
    carries through each run of ones from its lowest reached bit; towards lower bits the same on the reversed words."""
    m = (1 << bits) - 1

    def up(e_, r_):
        return r_ | ((((e_ + r_) & m) ^ e_) & e_)

    r = up(e, r)
    return brev_bits(up(brev_bits(e, bits), brev_bits(r, bits)), bits)


def fill_row_naive(e, r, bits):
    """The same by iteration: a bit of e beside a reached bit is reached, `bits` times over."""
    for _ in range(bits):
        r = (r | (r << 1) | (r >> 1)) & e & ((1 << bits) - 1)
    return r


_REV8 = np.array([int(format(i, "08b")[::-1], 2) for i in range(256)], np.uint8)
_ONE, _SHIFT63 = np.uint64(1), np.uint64(63)


def _brev64(a):
    b = np.ascontiguousarray(a, "<u8").view(np.uint8).reshape(a.shape + (8,))[..., ::-1]
    return np.ascontiguousarray(_REV8[b]).view("<u8").reshape(a.shape)


def _up64(e, r):
    return r | (((e + r) ^ e) & e)                                  # (uint64 arrays: the sum wraps)


def fill_row64(e, r):
    """fill_row_bits on uint64 arrays, as the kernel has it"""
    return _brev64(_up64(_brev64(e), _brev64(_up64(e, r))))


def pack_words(mask):
    """[rows, cols] bool -> [rows, W] uint64, bit x & 63 of word x >> 6; bits at or beyond cols are 0."""
    rows, cols = mask.shape
    W = (cols + 63) // 64
    padded = np.zeros((rows, W * 64), np.uint8)
    padded[:, :cols] = mask
    return np.packbits(padded.reshape(rows, W, 64), axis=-1, bitorder="little").view("<u8")[..., 0].copy()


def unpack_words(words, cols):
    a = np.ascontiguousarray(words, "<u8")
    bits = np.unpackbits(a.view(np.uint8).reshape(a.shape[0], a.shape[1], 8), axis=-1, bitorder="little")
    return bits.reshape(a.shape[0], -1)[:, :cols].astype(bool)


def _block_pass(e, old, new, bx, y0, c8):
    """One wave's work on planes padded by a zero word all round and to whole blocks (block (bx, y0) lies at [y0 + 1 : y0 + 65, bx + 1]):
    the block to its own fixpoint in "registers" against the halo of `old`, read once; stores into `new`; whether it changed."""
    E, r0 = e[y0 + 1:y0 + BLOCK + 1, bx + 1], old[y0 + 1:y0 + BLOCK + 1, bx + 1]
    col = old[y0:y0 + BLOCK + 2, bx + 1]
    side66 = (old[y0:y0 + BLOCK + 2, bx] >> _SHIFT63) | (old[y0:y0 + BLOCK + 2, bx + 2] << _SHIFT63)
    side = side66[1:-1]
    if not (r0.any() or side.any() or col[0] or col[-1] or (c8 and (side66[0] or side66[-1]))):
        return False                                                  # nothing reached in the block or around it
    side_ud = side66[:-2] | side66[2:]
    r = r0.copy()
    while True:
        ext = np.concatenate((col[:1], r, col[-1:]))
        v = ext[:-2] | ext[2:]
        if c8:
            v = v | (v << _ONE) | (v >> _ONE) | side_ud
        nxt = fill_row64(E, r | (E & (v | side)))
        if np.array_equal(nxt, r):
            break
        r = nxt
    if np.array_equal(r, r0):
        return False
    new[y0 + 1:y0 + BLOCK + 1, bx + 1] = r
    return True


def covered_tiled(original, wand):
    """(covered mask, passes): the bit planes, and Jacobi passes over all blocks until one changes nothing (that one is counted)."""
    x, y, tolerance, flags = (int(v) for v in wand[:4])
    rows, cols = original.shape[:2]
    em = eligible(original, x, y, tolerance)
    if flags & WAND_GLOBAL:
        return em, 0
    words = pack_words(em)
    W, R = words.shape[1], (rows + BLOCK - 1) // BLOCK * BLOCK
    assert not (words[:, -1] >> np.uint64((cols - 1) % 64) >> _ONE).any()          # nothing eligible at or beyond cols
    e = np.zeros((R + 2, W + 2), np.uint64)
    e[1:rows + 1, 1:W + 1] = words
    reach = np.zeros_like(e)
    reach[y + 1, (x >> 6) + 1] = np.uint64(1) << np.uint64(x & 63)
    passes = 0
    while True:
        passes += 1
        new = reach.copy()
        changed = [_block_pass(e, reach, new, bx, y0, bool(flags & WAND_CONNECT_8)) for y0 in range(0, R, BLOCK) for bx in range(W)]
        reach = new
        if not any(changed):
            return unpack_words(reach[1:rows + 1, 1:W + 1], cols), passes


# ---- shapes that make the schedule work ----------------------------------------------------------------------------------------------
INSIDE, WALL = (90, 100, 110), (200, 30, 60)


def from_mask(mask):
    """A BGR image that is INSIDE where the mask is set and WALL elsewhere: with a tolerance below 90 a seed inside selects the mask's component."""
    return np.where(mask[..., None], np.array(INSIDE, np.uint8), np.array(WALL, np.uint8)).astype(np.uint8)


def spiral(rows, cols):
    """A corridor one pixel wide that winds inwards from (0, 0) with one pixel of wall between its turns: the component is ONE long path."""
    m = np.zeros((rows, cols), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True

    def free(px, py, ddx, ddy):
        nx, ny, fx, fy = px + ddx, py + ddy, px + 2 * ddx, py + 2 * ddy
        return 0 <= nx < cols and 0 <= ny < rows and not m[ny, nx] and not (0 <= fx < cols and 0 <= fy < rows and m[fy, fx])

    while True:
        if not free(x, y, dx, dy):
            dx, dy = -dy, dx                                          # turn right (y grows downwards)
            if not free(x, y, dx, dy):
                return m
        x, y = x + dx, y + dy
        m[y, x] = True


def comb(rows, cols, direction):
    """A spine along one border and teeth one pixel wide, two apart, that reach almost across: entered from the spine, the teeth are walked
    leftwards ("left": the spine is the last column), rightwards, upwards or downwards."""
    m = np.zeros((rows, cols), bool)
    if direction in ("left", "right"):
        m[::2, 1:-1] = True
        m[:, -1 if direction == "left" else 0] = True
    else:
        m[1:-1, ::2] = True
        m[-1 if direction == "up" else 0, :] = True
    return m


def comb_seed(rows, cols, direction):
    return {"left": (cols - 1, 1), "right": (0, 1), "up": (1, rows - 1), "down": (1, 0)}[direction]


def quantised(rng, rows, cols):
    """A random image of three gray levels 12 apart, half of it in 3 x 3 patches and half per pixel, with one channel of every pixel
    lifted by 0..3: components of every size, and a Chebyshev distance that is not the gray one."""
    patches = rng.integers(0, 3, ((rows + 2) // 3, (cols + 2) // 3)).repeat(3, 0).repeat(3, 1)[:rows, :cols]
    level = np.where(rng.random((rows, cols)) < 0.5, patches, rng.integers(0, 3, (rows, cols)))
    img = (100 + 12 * level)[..., None].repeat(3, -1)
    img[np.arange(rows)[:, None], np.arange(cols)[None, :], rng.integers(0, 3, (rows, cols))] += rng.integers(0, 4, (rows, cols))
    return img.astype(np.uint8)


TOLERANCES = (15, 0, 3, 12, 2, 11)          # against `quantised`: 0..3 stay inside a level, 11 and 12 take part of the next one, 15 all of it


def random_wand(rng, rows, cols, kind, flags, seed=None, tol=None):
    """kind 0 a constant label, 1 a ramp, 2 an eraser; the tolerance (default: drawn) from those that separate the levels of `quantised`
    differently"""
    x, y = seed if seed is not None else (int(rng.integers(0, cols)), int(rng.integers(0, rows)))
    tol = int(rng.choice(TOLERANCES)) if tol is None else tol
    if kind == 2:
        return erase(x, y, tol, flags)
    axis = tuple(int(v) for v in (rng.integers(-20, cols + 20), rng.integers(-20, rows + 20), rng.integers(-20, cols + 20), rng.integers(-20, rows + 20)))
    l0 = int(rng.integers(0, 256))
    return (x, y, tol, flags) + axis + (l0, l0 if kind == 0 else int(rng.integers(0, 256)))


# ---- the call --------------------------------------------------------------------------------------------------------------------------
def info_of(mask):
    """(pixels, x0, y0, x1, y1) of rtdd_wand_info for a covered mask"""
    ys, xs = np.nonzero(mask)
    return int(mask.sum()), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def fill_similar(wand, edited, scribble, original, covered=covered_queue):
    """rtdd_fill_similar in place on edited [rows, cols, 3] and scribble [rows, cols]; returns info_of the covered set."""
    m = covered(original, wand)
    if isinstance(m, tuple):
        m = m[0]
    pr._write((0,) + tuple(wand[4:]), edited, scribble, original, 0, 0, m)
    return info_of(m)
