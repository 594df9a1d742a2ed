"""Sub-image views for the caller-memory tests: an image placed INSIDE a larger device allocation, the way a cv::cuda::GpuMat region of
interest hands one to the library -- a base pointer of any alignment class, any row stride, and somebody else's bytes all around it.

    parent (one allocation, its base what torch gives: at least 256-byte aligned)
    +---------------------------------------------------------------+
    |  >= 2 guard rows                                              |
    |  [16 + lead bytes][ row 0: width bytes ][ padding >= 16 bytes ]   <- one pitch
    |  [16 + lead bytes][ row 1               ][ padding            ]
    |  ...                                                          |
    |  >= 2 guard rows                                              |
    +---------------------------------------------------------------+

Column 0 of row 0 lies at `origin + lead_bytes`, origin a multiple of 256: lead_bytes IS the base pointer's alignment class.  The guards
keep every access a kernel could make within one pitch of a row, or 16 bytes either side of it, inside the allocation: these tests catch
wrong values and stray stores, never an access that leaves an allocation.

Everything outside the view is filled: inputs with 0xFF in every byte (NaN as f32, the Dirichlet label 255 as a scribble, the extreme
value as gray or BGR: one such byte that reaches a result changes it), outputs with a position-dependent byte pattern from a seeded
generator (no constant stray store matches it).  `result()` hands the view back after checking that fill; `assert_unchanged()` checks the
whole parent of an input.  Both checkers are plain numpy on a host copy of the parent (check_outside, check_unchanged), so that
tests/test_roi_util_cpu.py can test them without a GPU: Roi(..., device=None) keeps the parent in a numpy array.

A plain module -- no fixtures, no pytest settings."""
import numpy as np

GUARD_ROWS = 2
GUARD_BYTES = 16
FILL_INPUT = 0xFF                       # every byte outside (and, for assert_unchanged, the reference copy of) an input
FILL_OUTPUT = "pattern"                 # a seeded position-dependent byte pattern

# (lead_bytes, pitch residue): the pitch is the smallest multiple of 16 that holds the row and its guards, plus the residue.
# Chosen from the predicates the launchers test -- pointer % 4, pitch % 4 (u8 dword paths), pointer % 16, pitch % 16 (float4 paths):
#   u8:  leads 0..4; pitches = 0 mod 16, 0 mod 4 only, and 1, 2, 3 mod 4 (alternate rows change alignment);
#        an aligned pitch under an unaligned base, an unaligned pitch under an aligned base
#   f32: leads 0, 4, 8, 12; pitches = 0, 4, 8, 12 mod 16; a 16-byte pitch under a base that is 4- but not 16-byte aligned and the reverse
LAYOUTS_U8 = [(0, 0), (1, 0), (2, 4), (3, 1), (4, 2), (0, 3), (0, 1)]
LAYOUTS_F32 = [(0, 0), (4, 0), (8, 0), (12, 4), (0, 4), (0, 8), (0, 12)]


def pitch_for(width_bytes, lead_bytes, residue):
    """The row stride of a layout: room for the row, 16 guard bytes right of it and 16 + lead_bytes left of the next row."""
    return (width_bytes + 2 * GUARD_BYTES + lead_bytes + 15) // 16 * 16 + residue


class Geometry:
    """Where the view lies in the parent's bytes."""

    def __init__(self, rows, width, lead, pitch):
        assert pitch >= width + 2 * GUARD_BYTES + lead, "the pitch leaves no room for the guards"
        self.rows, self.width, self.lead, self.pitch = rows, width, lead, pitch
        self.left = GUARD_BYTES + lead                                       # bytes of a row's stride in front of its column 0
        self.origin = (GUARD_ROWS * pitch + self.left + 255) // 256 * 256    # a multiple of 256 with >= 2 rows + 16 + lead bytes in front
        self.first = self.origin + lead                                      # column 0 of row 0
        self.total = self.first + (rows + GUARD_ROWS) * pitch + GUARD_BYTES

    def view_mask(self):
        m = np.zeros(self.total, bool)
        for r in range(self.rows):
            m[self.first + r * self.pitch: self.first + r * self.pitch + self.width] = True
        return m

    def where(self, pos):
        """(row, byte, region) of parent byte `pos`: byte counts from the row's column 0 (negative in the lead), region is one of
        'view', 'padding', 'lead', 'guard rows above', 'guard rows below'."""
        rel = pos - self.first + self.left
        row, b = rel // self.pitch, rel % self.pitch - self.left
        if row < 0:
            region = "guard rows above"
        elif row >= self.rows:
            region = "guard rows below"
        else:
            region = "lead" if b < 0 else "view" if b < self.width else "padding"
        return int(row), int(b), region


def _report(geom, bad, what):
    pos = np.flatnonzero(bad)
    first = ", ".join("(row %d, byte %d: %s)" % geom.where(p) for p in pos[:6])
    return f"{what}: {len(pos)} bytes changed, first at {first}"


def check_outside(now, filled, geom, what="image"):
    """Every byte of `now` (the parent's bytes after a call) outside the view must equal `filled` (the parent as it was uploaded)."""
    bad = (now != filled) & ~geom.view_mask()
    assert not bad.any(), _report(geom, bad, f"{what}: written outside the view")


def check_unchanged(now, filled, geom, what="image"):
    """An input: the whole parent, view included, is what was uploaded."""
    bad = now != filled
    assert not bad.any(), _report(geom, bad, f"{what}: an input was modified")


class Roi:
    """A numpy image ([rows, cols] u8 or f32, or [rows, cols, 3] u8) inside a larger parent.  `lead_bytes`: the base pointer's alignment
    class; `pitch_bytes`: the row stride; `fill`: FILL_INPUT, FILL_OUTPUT or a byte value.  device=None: the parent is a numpy array."""

    def __init__(self, host, lead_bytes=0, pitch_bytes=None, fill=FILL_INPUT, device="cuda:0", seed=0, what="image"):
        host = np.ascontiguousarray(host)
        assert host.dtype in (np.uint8, np.float32) and host.ndim in (2, 3)
        self.shape, self.dtype, self.what = host.shape, host.dtype, what
        rows = host.shape[0]
        width = host.size // max(rows, 1) * host.itemsize if rows else 0
        if pitch_bytes is None:
            pitch_bytes = pitch_for(width, lead_bytes, 0)
        if host.dtype == np.float32:
            assert lead_bytes % 4 == 0 and pitch_bytes % 4 == 0, "an f32 image needs a 4-byte aligned pointer and pitch"
        self.geom = g = Geometry(rows, width, lead_bytes, pitch_bytes)
        if isinstance(fill, str):
            parent = np.random.default_rng(1000 + seed).integers(0, 256, g.total, dtype=np.uint8)
        else:
            parent = np.full(g.total, fill, np.uint8)
        rowsb = host.reshape(rows, -1).view(np.uint8) if rows else np.zeros((0, 0), np.uint8)
        for r in range(rows):
            parent[g.first + r * g.pitch: g.first + r * g.pitch + width] = rowsb[r]
        self.filled = parent                                   # the parent as uploaded: never modified
        self.pitch = pitch_bytes
        if device is None:
            self.base = parent.copy()
            self.ptr = None
        else:
            import torch
            self.base = torch.from_numpy(parent).to(device)
            assert self.base.data_ptr() % 256 == 0, "the allocator's base is less aligned than the layouts assume"
            self.ptr = self.base.data_ptr() + g.first

    @property
    def img(self):
        """What realtimedepthdiffusion_amd._img accepts: (pointer, pitch in bytes)."""
        return (self.ptr, self.pitch)

    def parent(self):
        """The parent's bytes now, on the host."""
        return self.base if isinstance(self.base, np.ndarray) else self.base.cpu().numpy()

    def _view(self, now):
        g = self.geom
        if g.rows == 0:
            return np.zeros(self.shape, self.dtype)
        idx = (g.first + np.arange(g.rows)[:, None] * g.pitch + np.arange(g.width)[None, :]).reshape(-1)
        return now[idx].view(self.dtype).reshape(self.shape)

    def result(self):
        """The view's pixels, after asserting that every parent byte outside the view still equals the fill."""
        now = self.parent()
        check_outside(now, self.filled, self.geom, self.what)
        return self._view(now)

    def assert_unchanged(self):
        check_unchanged(self.parent(), self.filled, self.geom, self.what)


def covering(*counts):
    """Index tuples over factors with counts[i] levels each in which every PAIR of levels of any two factors occurs: for up to n + 1
    factors of at most n levels, n the smallest prime >= max(counts), the rows (i, j, i + j, i + 2 j, ...) mod n of an orthogonal array,
    folded onto the levels a factor has.  Every single level and every pair stays; triples and beyond are what is dropped."""
    n = max(max(counts), len(counts) - 1, 2)
    while any(n % q == 0 for q in range(2, int(n ** 0.5) + 1)):
        n += 1
    out = []
    for i in range(n):
        for j in range(n):
            row = [i, j] + [(i + k * j) % n for k in range(1, len(counts) - 1)]
            t = tuple(v % c for v, c in zip(row, counts))
            if t not in out:
                out.append(t)
    return out
