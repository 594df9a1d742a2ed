"""Two restatements of rtdd_remove_object (include/rtdd.h) for the tests, which share no code: `remove` in vectorised numpy, level by level
(64-bit integers for the colours, float32 for the depth), and `remove_literal`, a per-pixel walk over the header's lines in Python
integers with numpy.float32 scalars.  Neither knows about the kernels: no tiles, no groups of levels, no apex -- every level of the chain
is a whole array.  Both return (artistic, depthOut); the depth of a pixel that is not filled is the input's, bit for bit.  `lift` restates
rtdd_lift_layer, and `nearest_in_row` is the fill the push-pull is measured against.  Test infrastructure."""
import numpy as np

F = np.float32
I64 = np.int64


def removal(select=0, grow=0, sourceMinDepth=0.0):
    """The fields of rtdd_removal as a dict; the float is rounded to f32 as the struct holds it."""
    return dict(select=int(select), grow=int(grow), sourceMinDepth=float(F(sourceMinDepth)))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def clamp_depth(depth):
    """d': NaN, -0 and everything below 0 are +0; everything above 255 is 255."""
    d = np.asarray(depth, F)
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, np.fmin(d, F(255)), F(0)).astype(F)


def selected(mask, select):
    return (mask != 0) if select == 0 else (mask == select)


def _dilate(sel, grow):
    """Pixels within Chebyshev distance `grow` of a True pixel of `sel` (the image's own pixels only)."""
    rows, cols = sel.shape
    p = np.zeros((rows, cols + 2 * grow), bool); p[:, grow:grow + cols] = sel
    a = np.zeros((rows + 2 * grow, cols), bool)
    for s in range(2 * grow + 1):
        a[grow:grow + rows] |= p[:, s:s + cols]
    out = np.zeros((rows, cols), bool)
    for s in range(2 * grow + 1):
        out |= a[s:s + rows]
    return out


def classes(depth, mask, R):
    """(hole, source) of level 0, two bool arrays; a pixel in neither is a bystander."""
    sel = selected(mask, R["select"])
    eligible = clamp_depth(depth) >= F(R["sourceMinDepth"])
    hole = sel | (eligible & _dilate(sel, R["grow"]))
    return hole, ~hole & eligible


def _pull(c, d, v):
    """One level up: c (r, k, 3) int64, d (r, k) f32, v (r, k) bool -> the same of ceil(r / 2) x ceil(k / 2)."""
    r, k = v.shape
    r2, k2 = (r + 1) // 2, (k + 1) // 2
    pc = np.zeros((2 * r2, 2 * k2, 3), I64); pc[:r, :k] = c
    pd = np.zeros((2 * r2, 2 * k2), F); pd[:r, :k] = d
    pv = np.zeros((2 * r2, 2 * k2), bool); pv[:r, :k] = v                  # a child that does not exist is not valid
    n = np.zeros((r2, k2), I64); sc = np.zeros((r2, k2, 3), I64); s = np.zeros((r2, k2), F); started = np.zeros((r2, k2), bool)
    for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cv, cd, cc = pv[a::2, b::2], pd[a::2, b::2], pc[a::2, b::2]
        n += cv
        sc += np.where(cv[..., None], cc, 0)
        added = s + cd
        assert added.dtype == F
        s = np.where(cv, np.where(started, added, cd), s)
        started |= cv
    valid = n > 0
    nn = np.maximum(n, 1)
    oc = np.where(valid[..., None], (2 * sc + nn[..., None]) // (2 * nn[..., None]), 0)
    od = np.where(valid, s / nn.astype(F), F(0))
    assert od.dtype == F
    return oc, od.astype(F), valid


def _push(c, d, v, cc, cd, cv):
    """The samples of (c, d, v) that are not valid, filled from the coarser level (cc, cd, cv).  Returns new (c, d, v)."""
    r, k = v.shape
    r2, k2 = cv.shape

    def taps(n, m):
        p = np.arange(n); near = p >> 1
        return near, np.clip(np.where(p & 1, near + 1, near - 1), 0, m - 1)
    yn, yf = taps(r, r2)
    xn, xf = taps(k, k2)
    g = lambda a, y, x: a[y][:, x]                                          # noqa: E731
    fc = (9 * g(cc, yn, xn) + 3 * g(cc, yn, xf) + 3 * g(cc, yf, xn) + g(cc, yf, xf) + 8) >> 4
    t = F(9) * g(cd, yn, xn)
    t = t + F(3) * g(cd, yn, xf)
    t = t + F(3) * g(cd, yf, xn)
    t = t + g(cd, yf, xf)
    fd = t * F(0.0625)
    assert fd.dtype == F
    fill = ~v & g(cv, yn, xn)
    return np.where(fill[..., None], fc, c), np.where(fill, fd, d).astype(F), v | fill


def fill_levels(c, d, v):
    """The push-pull on level-0 samples: returns (c, d, v) of level 0 after the push."""
    levels = [(c, d, v)]
    while levels[-1][2].shape != (1, 1):
        levels.append(_pull(*levels[-1]))
    cur = levels[-1]
    for lv in reversed(levels[:-1]):
        cur = _push(*lv, *cur)
    return cur


def remove(orig, depth, mask, R, counts=None):
    """rtdd_remove_object.  counts (a dict, optional) receives how many pixels were holes, filled, sources and bystanders."""
    orig = np.asarray(orig, np.uint8); depth = np.asarray(depth, F)
    hole, source = classes(depth, mask, R)
    c = np.where(source[..., None], orig.astype(I64), 0)
    d = np.where(source, clamp_depth(depth), F(0)).astype(F)
    fc, fd, fv = fill_levels(c, d, source)
    filled = hole & fv
    art = np.where(filled[..., None], fc, orig).astype(np.uint8)
    z = depth.copy()
    z[filled] = fd[filled]
    if counts is not None:
        counts.update(hole=int(hole.sum()), filled=int(filled.sum()), source=int(source.sum()), bystander=int((~hole & ~source).sum()))
    return art, z


# ---- the literal restatement: nothing above is used below ---------------------------------------------------------------------------

def remove_literal(orig, depth, mask, R, arity=None):
    """rtdd_remove_object pixel by pixel.  arity (a set, optional) receives every n > 0 a pull met."""
    rows, cols = mask.shape
    select, grow, smd = R["select"], R["grow"], F(R["sourceMinDepth"])

    def dprime(y, x):
        d = F(depth[y, x])
        if not d > F(0):
            return F(0)
        return F(255) if d > F(255) else d

    def is_selected(y, x):
        m = int(mask[y, x])
        return m != 0 if select == 0 else m == select

    def is_hole(y, x):
        if is_selected(y, x):
            return True
        if not dprime(y, x) >= smd:
            return False
        return any(is_selected(v, u) for v in range(max(y - grow, 0), min(y + grow, rows - 1) + 1)
                   for u in range(max(x - grow, 0), min(x + grow, cols - 1) + 1))

    hole = [[is_hole(y, x) for x in range(cols)] for y in range(rows)]
    # a sample: None (not valid) or (b, g, r, depth)
    level = [[None if hole[y][x] or not dprime(y, x) >= smd else (int(orig[y, x, 0]), int(orig[y, x, 1]), int(orig[y, x, 2]), dprime(y, x))
              for x in range(cols)] for y in range(rows)]
    chain = [level]
    while len(chain[-1]) > 1 or len(chain[-1][0]) > 1:
        fine = chain[-1]
        r, k = len(fine), len(fine[0])
        coarse = []
        for i in range((r + 1) // 2):
            row = []
            for j in range((k + 1) // 2):
                kids = [fine[2 * i + a][2 * j + b] for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)) if 2 * i + a < r and 2 * j + b < k]
                kids = [s for s in kids if s is not None]
                n = len(kids)
                if n == 0:
                    row.append(None)
                    continue
                if arity is not None:
                    arity.add(n)
                dsum = kids[0][3]
                for s in kids[1:]:
                    dsum = F(dsum + s[3])
                row.append(tuple((2 * sum(s[ch] for s in kids) + n) // (2 * n) for ch in range(3)) + (F(dsum / F(n)),))
            coarse.append(row)
        chain.append(coarse)
    for k in range(len(chain) - 2, -1, -1):
        fine, coarse = chain[k], chain[k + 1]
        r2, k2 = len(coarse), len(coarse[0])
        for y in range(len(fine)):
            yn = y >> 1
            yf = min(max(yn + 1 if y & 1 else yn - 1, 0), r2 - 1)
            for x in range(len(fine[0])):
                if fine[y][x] is not None or (k == 0 and not hole[y][x]):
                    continue
                xn = x >> 1
                xf = min(max(xn + 1 if x & 1 else xn - 1, 0), k2 - 1)
                if coarse[yn][xn] is None:
                    continue
                a, b, c, d = coarse[yn][xn], coarse[yn][xf], coarse[yf][xn], coarse[yf][xf]
                t = F(F(9) * a[3])
                t = F(t + F(F(3) * b[3]))
                t = F(t + F(F(3) * c[3]))
                t = F(t + d[3])
                fine[y][x] = tuple((9 * a[ch] + 3 * b[ch] + 3 * c[ch] + d[ch] + 8) >> 4 for ch in range(3)) + (F(t * F(0.0625)),)
    art = np.array(orig, np.uint8, copy=True)
    z = np.array(depth, F, copy=True)
    for y in range(rows):
        for x in range(cols):
            if hole[y][x] and chain[0][y][x] is not None:
                art[y, x] = chain[0][y][x][:3]
                z[y, x] = chain[0][y][x][3]
    return art, z


# ---- lift ---------------------------------------------------------------------------------------------------------------------------

def lift(orig, mask, select, x, y, srows, scols):
    """rtdd_lift_layer: the srows x scols x 4 sprite (B, G, R, A) whose texel (u, v) is image pixel (x + u, y + v)."""
    rows, cols = mask.shape
    sprite = np.zeros((srows, scols, 4), np.uint8)
    v0, v1 = max(0, -y), min(srows, rows - y)
    u0, u1 = max(0, -x), min(scols, cols - x)
    if v0 < v1 and u0 < u1:
        sel = selected(mask[y + v0:y + v1, x + u0:x + u1], select)
        sprite[v0:v1, u0:u1, :3] = np.where(sel[..., None], orig[y + v0:y + v1, x + u0:x + u1], 0)
        sprite[v0:v1, u0:u1, 3] = np.where(sel, 255, 0)
    return sprite


# ---- the fill it is measured against --------------------------------------------------------------------------------------------------

def nearest_in_row(orig, hole):
    """Every hole pixel takes the nearest pixel of its row that is no hole (the left one on a tie; a row that is all hole stays)."""
    out = orig.copy()
    cols = hole.shape[1]
    x = np.arange(cols)
    for y in np.nonzero(hole.any(1))[0]:
        good = x[~hole[y]]
        if good.size == 0:
            continue
        pos = np.clip(np.searchsorted(good, x), 0, good.size - 1)
        left = good[np.maximum(pos - 1, 0)]; right = good[pos]
        near = np.where(np.abs(x - left) <= np.abs(right - x), left, right)
        out[y, hole[y]] = orig[y, near[hole[y]]]
    return out


# ---- the masks the tests share ------------------------------------------------------------------------------------------------------

CODE, OTHER = 7, 9                      # the region code the tests select, and another one (selected too when select == 0)
PATTERNS = ["random", "checker", "borders", "all", "none", "allbut", "disc"]


def mask_pattern(name, rows, cols, seed=0):
    """A u8 mask: CODE where the pattern is, 0 elsewhere; "random" also scatters OTHER over 10 % of the rest."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if name == "random":
        m = np.where(rng.random((rows, cols)) < 0.5, CODE, 0)
        m = np.where((m == 0) & (rng.random((rows, cols)) < 0.1), OTHER, m)
    elif name == "checker":
        m = np.where((yy + xx) & 1, CODE, 0)
    elif name == "borders":                                              # a block in each corner and one on each edge
        a, b = max(rows // 5, 1), max(cols // 5, 1)
        ym, xm = rows // 2, cols // 2
        edge_y = (yy < a) | (yy >= rows - a); edge_x = (xx < b) | (xx >= cols - b)
        m = np.where((edge_y & edge_x) | (edge_y & (abs(xx - xm) <= b // 2)) | (edge_x & (abs(yy - ym) <= a // 2)), CODE, 0)
    elif name == "all":
        m = np.full((rows, cols), CODE)
    elif name == "none":
        m = np.zeros((rows, cols), int)
    elif name == "allbut":
        m = np.full((rows, cols), CODE); m[0, 0] = 0
    elif name == "disc":                                                 # one disc, 0.4 of the smaller side in radius, off centre
        r = 0.4 * min(rows, cols)
        m = np.where((yy - rows * 0.45) ** 2 + (xx - cols * 0.55) ** 2 <= r * r, CODE, 0)
    else:
        raise ValueError(name)
    return m.astype(np.uint8)
