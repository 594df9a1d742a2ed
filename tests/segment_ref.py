"""rtdd_segment_surfaces restated (include/rtdd.h, "every surface of the depth map in one call"): test infrastructure.

A segmentation is the 7-tuple (step, lo, hi, minPixels, maxRegions, firstCode, flags) of rtdd_segmentation.  A label map is an int32 array
[rows, cols]: the smallest linear index y * cols + x of the pixel's component, -1 where the pixel is inadmissible.  Routes to it that share
no code: `labels_unionfind` (a union-find over Python integers, the rule evaluated per pixel), `labels_queue` (an explicit queue from every
unvisited pixel over surface_ref.clamped), `labels_ndimage` (scipy.ndimage.label, where step = 255 makes a link mere admissibility),
`labels_graph` (scipy's connected components over the vectorised link list: the fast one the GPU tests use) and `labels_tiled`, which
restates the kernels' structure from the exported constants: runs of H links labelled by bit arithmetic, V links united inside a tile,
the links across tile borders united on the global parents, both with the skipped unions, then flattened.  tests/test_segment_cpu.py pins
them against each other.  Then the ranking, the records, the writes."""
from collections import deque

import numpy as np

import realtimedepthdiffusion_amd as rt
import surface_ref as sf
import wand_ref as wr

f32 = np.float32
TILE_W, TILE_H, HEAD = rt.SEGMENT_TILE_W, rt.SEGMENT_TILE_H, rt.SEGMENT_HEAD


def seg(step, lo=0, hi=255, min_pixels=1, max_regions=255, first_code=1, flags=0):
    return (step, lo, hi, min_pixels, max_regions, first_code, flags)


def valid(s):
    """what rtdd_segment_surfaces accepts in the struct"""
    step, lo, hi, min_pixels, max_regions, first_code, flags = s
    return (all(np.isfinite(v) and 0 <= v <= 255 for v in (step, lo, hi)) and lo <= hi and min_pixels >= 1 and 1 <= max_regions <= 255
            and 1 <= first_code <= 255 and first_code + max_regions - 1 <= 255 and flags == 0)


# ---- route 1: a union-find over Python integers --------------------------------------------------------------------------------------------
def labels_unionfind(depth, s):
    step, lo, hi = f32(s[0]), f32(s[1]), f32(s[2])
    d = np.asarray(depth, f32)
    rows, cols = d.shape

    def dprime(v):                                                    # d > 0 ? fminf(d, 255) : +0, on one value
        return min(v, f32(255)) if v > 0 else f32(0)

    dc = [[dprime(d[y, x]) for x in range(cols)] for y in range(rows)]
    adm = [[bool(lo <= v) and bool(v <= hi) for v in row] for row in dc]
    parent = list(range(rows * cols))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for y in range(rows):
        for x in range(cols):
            if not adm[y][x]:
                continue
            if x + 1 < cols and adm[y][x + 1] and bool(abs(f32(dc[y][x] - dc[y][x + 1])) <= step):
                unite(y * cols + x, y * cols + x + 1)
            if y + 1 < rows and adm[y + 1][x] and bool(abs(f32(dc[y][x] - dc[y + 1][x])) <= step):
                unite(y * cols + x, (y + 1) * cols + x)
    return np.array([[find(y * cols + x) if adm[y][x] else -1 for x in range(cols)] for y in range(rows)], np.int32).reshape(rows, cols)


# ---- route 2: an explicit queue from every unvisited pixel, in linear order ------------------------------------------------------------------
def labels_queue(depth, s):
    step, lo, hi = f32(s[0]), f32(s[1]), f32(s[2])
    dc = sf.clamped(depth)
    rows, cols = dc.shape
    adm = lambda v: bool(lo <= v) and bool(v <= hi)
    out = np.full((rows, cols), -1, np.int32)
    for y in range(rows):
        for x in range(cols):
            if out[y, x] >= 0 or not adm(dc[y, x]):
                continue
            root = y * cols + x                                       # the first pixel met in linear order is the smallest index
            out[y, x] = root
            todo = deque([(x, y)])
            while todo:
                px, py = todo.popleft()
                p = dc[py, px]
                for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    qx, qy = px + dx, py + dy
                    if not (0 <= qx < cols and 0 <= qy < rows) or out[qy, qx] >= 0:
                        continue
                    q = dc[qy, qx]
                    if adm(q) and bool(np.abs(f32(p - q)) <= step):
                        out[qy, qx] = root
                        todo.append((qx, qy))
    return out


def _roots_of(lab, member):
    """a map of arbitrary component numbers (valid where `member`) -> the smallest linear index of each component, -1 elsewhere"""
    rows, cols = lab.shape
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    smallest = np.full(int(lab.max()) + 1, rows * cols, np.int64)
    np.minimum.at(smallest, lab[member], idx[member])
    return np.where(member, smallest[lab], -1).astype(np.int32)


# ---- route 3: scipy.ndimage.label, where a link is mere admissibility -------------------------------------------------------------------------
def labels_ndimage(depth, s):
    from scipy import ndimage
    assert s[0] == 255, "only where no step separates two admissible neighbours"
    dc = sf.clamped(depth)
    a = (f32(s[1]) <= dc) & (dc <= f32(s[2]))
    lab, _ = ndimage.label(a, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return _roots_of(lab, a)


# ---- the fast one: the vectorised link list ------------------------------------------------------------------------------------------------
def planes(depth, s):
    """(A, H, V) as bool [rows, cols]: admissible; the link to the right; the link downwards"""
    dc = sf.clamped(depth)
    step, lo, hi = f32(s[0]), f32(s[1]), f32(s[2])
    a = (lo <= dc) & (dc <= hi)
    H, V = np.zeros(dc.shape, bool), np.zeros(dc.shape, bool)
    H[:, :-1] = a[:, :-1] & a[:, 1:] & (np.abs(dc[:, :-1] - dc[:, 1:]) <= step)
    V[:-1, :] = a[:-1, :] & a[1:, :] & (np.abs(dc[:-1, :] - dc[1:, :]) <= step)
    return a, H, V


def labels_graph(depth, s):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a, H, V = planes(depth, s)
    rows, cols = a.shape
    idx = np.arange(rows * cols).reshape(rows, cols)
    p = np.concatenate((idx[H], idx[V]))
    q = np.concatenate((idx[H] + 1, idx[V] + cols))
    g = coo_matrix((np.ones(len(p), np.int8), (p, q)), shape=(rows * cols, rows * cols))
    _, lab = connected_components(g, directed=False)
    return _roots_of(lab.reshape(rows, cols), a)


# ---- the kernels' structure ----------------------------------------------------------------------------------------------------------------
def run_start_bits(h, lane, bits):
    """seg_run_start on words of `bits` bits: the first pixel of the run of links (bit x of h: x - x + 1) that holds pixel `lane`: one above
    the highest missing link below it."""
    m = ~h & ((1 << lane) - 1) & ((1 << bits) - 1)
    return m.bit_length()                                             # (64 - clz on the device; 0 where m == 0)


def run_start_naive(h, lane, bits):
    while lane > 0 and (h >> (lane - 1)) & 1:
        lane -= 1
    return lane


def implied_bits(v, h, hbelow, bits):
    """seg_implied: the V links whose union the pair to their left implies"""
    return ((v & h & hbelow) << 1) & ((1 << bits) - 1)


def implied_naive(v, h, hbelow, bits):
    return sum(1 << x for x in range(1, bits) if (v >> (x - 1)) & 1 and (h >> (x - 1)) & 1 and (hbelow >> (x - 1)) & 1)


def labels_tiled(depth, s, stats=None):
    """The device's four steps on the packed planes.  `stats` (a dict) receives the number of unions made inside tiles and across
    borders, and of those skipped as implied."""
    a, Hm, Vm = planes(depth, s)
    rows, cols = a.shape
    A, H, V = (wr.pack_words(m).tolist() for m in (a, Hm, Vm))        # [rows][W] Python integers
    W = len(A[0])
    P = [-1] * (rows * cols)
    count = {"local": 0, "border": 0, "skipped": 0}

    def find(par, i):
        while par[i] != i:
            i = par[i]
        return i

    def unite(par, p, q):
        p, q = find(par, p), find(par, q)
        if p != q:
            par[max(p, q)] = min(p, q)

    # k_segment_local
    for ty0 in range(0, rows, TILE_H):
        for bx in range(W):
            L = [-1] * (TILE_W * TILE_H)
            th = min(TILE_H, rows - ty0)
            for r in range(th):
                for lane in range(TILE_W):
                    if (A[ty0 + r][bx] >> lane) & 1:
                        L[r * TILE_W + lane] = r * TILE_W + run_start_bits(H[ty0 + r][bx], lane, 64)
            for r in range(th - 1):
                y = ty0 + r
                v = V[y][bx]
                todo = v & ~implied_bits(v, H[y][bx], H[y + 1][bx], 64)
                count["skipped"] += bin(v & ~todo).count("1")
                for lane in range(TILE_W):
                    if (todo >> lane) & 1:
                        unite(L, r * TILE_W + lane, (r + 1) * TILE_W + lane)
                        count["local"] += 1
            for r in range(th):
                for lane in range(TILE_W):
                    x = bx * TILE_W + lane
                    if x < cols and L[r * TILE_W + lane] >= 0:
                        root = find(L, r * TILE_W + lane)
                        P[(ty0 + r) * cols + x] = (ty0 + root // TILE_W) * cols + bx * TILE_W + root % TILE_W
    # k_segment_merge
    for ty0 in range(0, rows, TILE_H):
        for bx in range(W):
            yb = ty0 + TILE_H - 1
            if yb + 1 < rows:
                v = V[yb][bx]
                todo = v & ~implied_bits(v, H[yb][bx], H[yb + 1][bx], 64)
                count["skipped"] += bin(v & ~todo).count("1")
                for lane in range(TILE_W):
                    if (todo >> lane) & 1:
                        p = yb * cols + bx * TILE_W + lane
                        unite(P, p, p + cols)
                        count["border"] += 1
            if bx + 1 < W:
                for y in range(ty0, min(ty0 + TILE_H, rows)):
                    if H[y][bx] >> 63:
                        if y > 0 and H[y - 1][bx] >> 63 and V[y - 1][bx] >> 63 and V[y - 1][bx + 1] & 1:
                            count["skipped"] += 1
                            continue
                        p = y * cols + bx * TILE_W + 63
                        unite(P, p, p + 1)
                        count["border"] += 1
    if stats is not None:
        stats.update(count)
    # k_segment_flatten
    return np.array([find(P, i) if P[i] >= 0 else -1 for i in range(rows * cols)], np.int32).reshape(rows, cols)


# ---- the ranking, the records, the writes -------------------------------------------------------------------------------------------------
def rank(labels, s):
    """(components, candidates, [(root, size), ...] of the regions in rank order)"""
    roots, sizes = np.unique(labels[labels >= 0], return_counts=True)
    cand = [(int(r), int(n)) for r, n in zip(roots, sizes) if n >= s[3]]
    cand.sort(key=lambda c: (-c[1], c[0]))
    return len(roots), len(cand), cand[:s[4]]


def segment(depth, s, labels=labels_graph):
    """(label map, info (components, candidates, regions, pixels), records): a record is (code, pixels, rootX, rootY, x0, y0, x1, y1,
    bits of dmin, bits of dmax)."""
    lab = labels(depth, s)
    rows, cols = lab.shape
    dc = sf.clamped(depth)
    components, candidates, regions = rank(lab, s)
    records = []
    for k, (root, size) in enumerate(regions):
        m = lab == root
        ys, xs = np.nonzero(m)
        records.append((s[5] + k, size, root % cols, root // cols, int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()),
                        int(dc[m].min().view(np.uint32)), int(dc[m].max().view(np.uint32))))
    return lab, (components, candidates, len(regions), sum(r[1] for r in records)), records


def write(lab, records, cols, edited, scribble):
    """the writes of the regions on a pair, in place"""
    for rec in records:
        m = lab == rec[3] * cols + rec[2]
        edited[m] = rec[0]
        scribble[m] = 255


def segment_surfaces(s, edited, scribble, depth, labels=labels_graph):
    """rtdd_segment_surfaces in place on edited [rows, cols, 3] and scribble [rows, cols] (both None: nothing painted); returns
    (label map, info, records)."""
    lab, info, records = segment(depth, s, labels)
    if edited is not None:
        write(lab, records, lab.shape[1], edited, scribble)
    return lab, info, records


def record_of(r):
    """an rt.Segment as the tuple above"""
    return (r.code, r.pixels, r.rootX, r.rootY, r.x0, r.y0, r.x1, r.y1, int(np.float32(r.dmin).view(np.uint32)), int(np.float32(r.dmax).view(np.uint32)))


def info_of(i):
    return (i.components, i.candidates, i.regions, i.pixels)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
def six_fields():
    """the six fields drawn in order from default_rng(10), one for each step of STEPS ascending"""
    rng = np.random.default_rng(10)
    return [(step, sf.field(rng, 67, 45)) for step in sorted(sf.STEPS)]


def u_shape():
    """two arms that lie in one tile and meet only in the tile below: two tile-local labels that must become one"""
    m = np.zeros((2 * TILE_H + 3, 40), bool)
    m[2:TILE_H + 4, 5] = m[2:TILE_H + 4, 20] = True
    m[TILE_H + 3, 5:21] = True
    return m


def rings(rows=60, cols=150):
    yy, xx = np.mgrid[:rows, :cols]
    r = np.maximum(np.abs(yy - rows // 2), np.abs(xx - cols // 2) * rows // cols)
    return (f32(20) + f32(10) * (r // 4)).astype(f32)                # square rings four pixels wide, 10 apart in depth


def ranking_map():
    """sizes 4, 4, 3, 3, 3, 2, 2, 1, 1, 1 on an inadmissible background: roots decide among equal sizes"""
    rows = ["AAA.BBB.CCC",
            "...........",
            "DD.EE.F.G..",
            "...........",
            "HHHH.IIII.J"]
    depth = np.array([[200 if ch == "." else 10 * (ord(ch) - 64) for ch in row] for row in rows], f32)
    return depth, [44, 49, 0, 4, 8, 22, 25, 28, 30, 54]


def scene():
    """test_fill_surface_cpu's 48 x 40 ellipse (513 pixels, in three parts there) at depth 60, a box at 120, the background at 200, and a
    few stray pixels that are components of their own"""
    rows, cols = 48, 80
    yy, xx = np.mgrid[:rows, :cols]
    obj = ((yy - 24) / 15) ** 2 + ((xx - 20) / 11) ** 2 <= 1
    assert obj.sum() == 513
    box = (yy >= 10) & (yy < 30) & (xx >= 50) & (xx < 72)
    depth = np.where(obj, f32(60), np.where(box, f32(120), f32(200))).astype(f32)
    depth[20:30, 50:72][:, ::7] += f32(2)                             # a box that is not flat
    for y, x, v in ((3, 3, 90), (40, 60, 10), (24, 20, 75), (24, 21, 75), (15, 60, 140)):
        depth[y, x] = v
    return depth, obj, box
