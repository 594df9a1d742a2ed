// remove.hip -- an object taken out of the scene (rtdd_remove_object, rtdd_lift_layer, include/rtdd.h; DESIGN.md section 4 "Remove"):
// the selection is filled, colour and depth, by a push-pull over a pyramid, or cut out as a sprite for rtdd_composite_layer.
//
// The rule is the header's, level by level; a launch per level each way would be launch latency and nothing else, so the levels go in
// GROUPS of kRemoveGroup = 3, and no level inside a group is ever stored:
//   k_remove_pull   a workgroup owns a 64 x 64 tile of a level (level 0: the images, classified here), reduces three levels in LDS and
//                   stores the 8 x 8 samples of the third to the context's table buffer.  The same kernel reads stored samples where
//                   the image needs a further group.
//   k_remove_apex   ONE workgroup: a stored level of at most kRemoveApex samples goes to 1 x 1 and back down, the whole chain in LDS;
//                   the filled level is stored beside the pulled one (the pulled one is read again below, so it is kept).
//   k_remove_push   a workgroup owns the same tile: it reads the filled coarse level with a one-sample halo, pulls the tile's two
//                   intermediate levels again in LDS (with the halo the push needs: 72 x 72 samples of the tile's level), pushes down
//                   and writes the outputs.  A tile without a hole copies, four pixels per lane, and touches no LDS beyond the test.
// 2 P + 1 launches for P groups: 3 while ceil(rows / 8) * ceil(cols / 8) <= kRemoveApex, 5 up to 8K and beyond.
//
// A sample is 8 bytes: b | g << 8 | r << 16 | valid << 24, and the depth.  Integers are exact; the floats are single operations: this
// translation unit is compiled with -ffp-contract=off and holds no fmaf, `/` is the correctly rounded one -- the bytes and the depth's
// bits are those of tests/remove_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.  No atomics; every output is stored exactly once.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

constexpr int kT = kRemoveTile, kG = kRemoveGroup;
constexpr int kHalo = 1 << (kG - 1);                  // 4: what the push needs of the tile's own level around the tile
constexpr int kR = kT + 2 * kHalo;                    // 72: the side of that region
constexpr int kMaxGrow = 8;
constexpr int kThreads = 256;
constexpr uint32_t kValid = 1u << 24;
static_assert(kT == 64 && kG == 3, "the LDS regions below are sized for 64 / 3");

struct Stored { uint2 *p; int rows, cols; };          // a level in the table buffer, rows x cols samples, dense
struct Region { int oy, ox, n; };                     // an n x n window of a level held in LDS; (oy, ox): the level's sample at its corner

// level 0 as the caller's images
struct Images {
    const uint8_t *orig; size_t op;
    const float *depth; size_t dp;
    const uint8_t *mask; size_t mp;
    int select, grow;
    float minDepth;
};

// idx / n for 0 <= idx < 2^24 and 2 <= n < 256 by one multiplication: inv = ceil(2^32 / n), and idx * (inv * n - 2^32) < 2^32
struct Div {
    uint32_t inv; int n;
    __device__ __forceinline__ explicit Div(int n_) : inv(0xffffffffu / (uint32_t)n_ + 1u), n(n_) {}
    __device__ __forceinline__ int quot(int idx) const { return (int)__umulhi((uint32_t)idx, inv); }
};

__device__ __forceinline__ bool is_selected(uint32_t m, int select) { return select == 0 ? m != 0u : m == (uint32_t)select; }

// ---- classes of level 0 over an S x S window at (oy, ox), which may reach outside the image: 0 bystander or outside, 1 source, 2 hole.
// selb: (S + 2 grow)^2 bytes, rowd: (S + 2 grow) * S bytes, flags: S * S bytes.  Ends with a barrier.
// GROW false: grow == 0, one pass and no halo.
template <int S, bool GROW>
__device__ void classify(const Images &im, int rows, int cols, int oy, int ox, uint8_t *selb, uint8_t *rowd, uint8_t *flags) {
    if (!GROW) {
#pragma unroll 4
        for (int idx = threadIdx.x; idx < S * S; idx += kThreads) {
            const int i = idx / S, j = idx - i * S, y = oy + i, x = ox + j;
            uint8_t f = 0;
            if (y >= 0 && y < rows && x >= 0 && x < cols) {
                const bool sel = is_selected(im.mask[(size_t)y * im.mp + x], im.select);
                const float d = remove_depth(*(const float *)((const char *)im.depth + (size_t)y * im.dp + 4 * (size_t)x));
                f = sel ? 2 : (d >= im.minDepth ? 1 : 0);
            }
            flags[idx] = f;
        }
        __syncthreads();
        return;
    }
    const int g = im.grow, W = S + 2 * g;
    const Div dw(W);
#pragma unroll 4
    for (int idx = threadIdx.x; idx < W * W; idx += kThreads) {
        const int i = dw.quot(idx), j = idx - i * W, y = oy - g + i, x = ox - g + j;
        uint8_t s = 0;
        if (y >= 0 && y < rows && x >= 0 && x < cols) s = is_selected(im.mask[(size_t)y * im.mp + x], im.select);
        selb[idx] = s;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < W * S; idx += kThreads) {
        const int i = idx / S, j = idx - i * S;
        uint8_t r = 0;
        for (int s = 0; s <= 2 * g; s++) r |= selb[i * W + j + s];
        rowd[idx] = r;
    }
    __syncthreads();
#pragma unroll 2
    for (int idx = threadIdx.x; idx < S * S; idx += kThreads) {
        const int i = idx / S, j = idx - i * S, y = oy + i, x = ox + j;
        uint8_t f = 0;
        if (y >= 0 && y < rows && x >= 0 && x < cols) {
            uint8_t near = 0;
            for (int s = 0; s <= 2 * g; s++) near |= rowd[(i + s) * S + j];
            const float d = remove_depth(*(const float *)((const char *)im.depth + (size_t)y * im.dp + 4 * (size_t)x));
            const bool eligible = d >= im.minDepth;
            f = (selb[(i + g) * W + j + g] || (eligible && near)) ? 2 : (eligible ? 1 : 0);
        }
        flags[idx] = f;
    }
    __syncthreads();
}

// ---- where a pull reads its children: each returns whether sample (y, x), y, x >= 0, exists and is valid, and then its colour and depth
struct FromImages {
    const Images &im; const uint8_t *flags; Region r; int rows, cols;
    __device__ __forceinline__ bool operator()(int y, int x, uint32_t &c, float &d) const {
        const int i = y - r.oy, j = x - r.ox;
        if (y >= rows || x >= cols || (unsigned)i >= (unsigned)r.n || (unsigned)j >= (unsigned)r.n || flags[i * r.n + j] != 1) return false;
        c = load_bgr(im.orig + (size_t)y * im.op + 3 * (size_t)x);
        d = remove_depth(*(const float *)((const char *)im.depth + (size_t)y * im.dp + 4 * (size_t)x));
        return true;
    }
};
struct FromStored {
    Stored s;
    __device__ __forceinline__ bool operator()(int y, int x, uint32_t &c, float &d) const {
        if (y >= s.rows || x >= s.cols) return false;
        const uint2 v = s.p[(size_t)y * s.cols + x];
        c = v.x & 0xffffffu; d = __uint_as_float(v.y);
        return (v.x & kValid) != 0u;
    }
};
struct FromLds {
    const uint32_t *c_; const float *d_; Region r; int rows, cols;
    __device__ __forceinline__ bool operator()(int y, int x, uint32_t &c, float &d) const {
        const int i = y - r.oy, j = x - r.ox;
        if (y >= rows || x >= cols || (unsigned)i >= (unsigned)r.n || (unsigned)j >= (unsigned)r.n) return false;
        const uint32_t v = c_[i * r.n + j];
        c = v & 0xffffffu; d = d_[i * r.n + j];
        return (v & kValid) != 0u;
    }
};

// PULL: sample (i, j) of the coarser level from the children `src` finds.  Returns the packed colour (0: not valid) and the depth.
template <class Src>
__device__ __forceinline__ uint32_t pull_sample(const Src &src, int i, int j, float &depth) {
    uint32_t n = 0, sb = 0, sg = 0, sr = 0;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {                                   // (0,0), (0,1), (1,0), (1,1)
        uint32_t c; float d;
        if (src(2 * i + (k >> 1), 2 * j + (k & 1), c, d)) {
            s = n ? s + d : d;
            n++; sb += c & 255u; sg += (c >> 8) & 255u; sr += (c >> 16) & 255u;
        }
    }
    depth = 0.0f;
    if (!n) return 0u;
    // s / (float)n and (2 sum + n) div (2 n): n = 1, 2, 4 are exact scalings and shifts (the same bits as the divisions), n = 3 divides
    depth = n == 3u ? s / 3.0f : s * (n == 1u ? 1.0f : n == 2u ? 0.5f : 0.25f);
    auto avg = [&](uint32_t sum) { const uint32_t v = 2u * sum + n; return n == 1u ? v >> 1 : n == 2u ? v >> 2 : n == 4u ? v >> 3 : v / 6u; };
    return avg(sb) | (avg(sg) << 8) | (avg(sr) << 16) | kValid;
}

// a region of a level of lrows x lcols samples pulled from `src`; samples of the region outside the level are not valid
template <class Src>
__device__ void pull_region(const Src &src, Region r, int lrows, int lcols, uint32_t *oc, float *od, int nthreads) {
    const Div dn(r.n);
#pragma unroll 2
    for (int idx = threadIdx.x; idx < r.n * r.n; idx += nthreads) {
        const int q = dn.quot(idx), i = r.oy + q, j = r.ox + idx - q * r.n;
        uint32_t c = 0u; float d = 0.0f;
        if (i >= 0 && i < lrows && j >= 0 && j < lcols) c = pull_sample(src, i, j, d);
        oc[idx] = c; od[idx] = d;
    }
}

// PUSH, the header's line: the near and the far tap of coordinate p in a coarse level of m samples along that axis ...
__device__ __forceinline__ void push_taps(int p, int m, int &near, int &far) {
    near = p >> 1;
    far = min(max((p & 1) ? near + 1 : near - 1, 0), m - 1);
}
// ... and the sample from the four taps at rows in / iff and columns jn / jf of a window of `pitch` samples a row.  Returns the packed
// colour, 0 if [yn, xn] is not valid.  The only statement of the push's arithmetic in this file.
__device__ __forceinline__ uint32_t push_blend(const uint32_t *cc, const float *cd, int pitch, int in, int iff, int jn, int jf, float &depth) {
    const uint32_t a = cc[in * pitch + jn], b = cc[in * pitch + jf], c = cc[iff * pitch + jn], e = cc[iff * pitch + jf];
    depth = 0.0f;
    if (!(a & kValid)) return 0u;
    float t = 9.0f * cd[in * pitch + jn];
    t = t + 3.0f * cd[in * pitch + jf];
    t = t + 3.0f * cd[iff * pitch + jn];
    t = t + cd[iff * pitch + jf];
    depth = t * 0.0625f;
    uint32_t out = kValid;
#pragma unroll
    for (int s = 0; s < 24; s += 8)
        out |= ((9u * ((a >> s) & 255u) + 3u * ((b >> s) & 255u) + 3u * ((c >> s) & 255u) + ((e >> s) & 255u) + 8u) >> 4) << s;
    return out;
}

// Sample (y, x) of a level from the coarser level of crows x ccols samples held as region rc.  0 too if a tap lies outside rc (only
// samples the tile never reads: the outer ring of a halo).
__device__ __forceinline__ uint32_t push_sample(const uint32_t *cc, const float *cd, Region rc, int crows, int ccols, int y, int x, float &depth) {
    int yn, yf, xn, xf;
    push_taps(y, crows, yn, yf); push_taps(x, ccols, xn, xf);
    const int in = yn - rc.oy, jf = xf - rc.ox, jn = xn - rc.ox, iff = yf - rc.oy;
    depth = 0.0f;
    if ((unsigned)in >= (unsigned)rc.n || (unsigned)iff >= (unsigned)rc.n || (unsigned)jn >= (unsigned)rc.n || (unsigned)jf >= (unsigned)rc.n) return 0u;
    return push_blend(cc, cd, rc.n, in, iff, jn, jf, depth);
}

// the samples of region rf (a level of frows x fcols) that are not valid, filled in place from the coarser region
__device__ void push_region(Region rf, uint32_t *fc, float *fd, int frows, int fcols, Region rc, const uint32_t *cc, const float *cd, int crows, int ccols,
                            int nthreads) {
    const Div dn(rf.n);
    for (int idx = threadIdx.x; idx < rf.n * rf.n; idx += nthreads) {
        const int q = dn.quot(idx), y = rf.oy + q, x = rf.ox + idx - q * rf.n;
        if (y < 0 || y >= frows || x < 0 || x >= fcols || (fc[idx] & kValid)) continue;
        float d;
        const uint32_t c = push_sample(cc, cd, rc, crows, ccols, y, x, d);
        if (c) { fc[idx] = c; fd[idx] = d; }
    }
}

__device__ __forceinline__ int half_up(int v, int times) { for (int i = 0; i < times; i++) v = (v + 1) >> 1; return v; }

// The LDS of the two tile kernels: the window's classes and the three coarser levels of a group, with the push's halo.
struct TileLds {
    uint8_t selb[(kR + 2 * kMaxGrow) * (kR + 2 * kMaxGrow)], rowd[(kR + 2 * kMaxGrow) * kR], flags[kR * kR];
    uint32_t c1[36 * 36], c2[18 * 18], c3[10 * 10];
    float d1[36 * 36], d2[18 * 18], d3[10 * 10];
};

// ---- k_remove_pull: tile (blockIdx.y, blockIdx.x) of a level of rows x cols samples -- IMAGE: the images, else `src` -- reduced g <= 3
// levels; the last is stored into dst (g == 0, a 1 x 1 image: the level itself).
template <bool IMAGE, bool GROW>
__global__ __launch_bounds__(kThreads) void k_remove_pull(Images im, Stored src, Stored dst, int rows, int cols, int g) {
    __shared__ TileLds L;
    const int ty = blockIdx.y * kT, tx = blockIdx.x * kT;
    const Region r0 = {ty, tx, kT};
    if (IMAGE) classify<kT, GROW>(im, rows, cols, ty, tx, L.selb, L.rowd, L.flags);
    uint32_t *lc[4]; float *ld[4];
    lc[0] = nullptr; lc[1] = L.c1; lc[2] = L.c2; lc[3] = L.c3;
    ld[0] = nullptr; ld[1] = L.d1; ld[2] = L.d2; ld[3] = L.d3;
    const FromImages fi = {im, L.flags, r0, rows, cols};
    const FromStored fs = {src};
    if (g == 0) {                                                   // rows == cols == 1
        if (threadIdx.x == 0) {
            uint32_t c = 0u; float d = 0.0f;
            const bool v = IMAGE ? fi(0, 0, c, d) : fs(0, 0, c, d);
            dst.p[0] = make_uint2(v ? (c | kValid) : 0u, __float_as_uint(v ? d : 0.0f));
        }
        return;
    }
    int lr = rows, lcn = cols;
    Region rj = r0;
    for (int j = 1; j <= g; j++) {
        const Region fine = rj;
        const int fr = lr, fcn = lcn;
        lr = (lr + 1) >> 1; lcn = (lcn + 1) >> 1;
        rj = {ty >> j, tx >> j, kT >> j};
        if (j == 1) {
            if (IMAGE) pull_region(fi, rj, lr, lcn, lc[1], ld[1], kThreads);
            else pull_region(fs, rj, lr, lcn, lc[1], ld[1], kThreads);
        } else {
            const FromLds fl = {lc[j - 1], ld[j - 1], fine, fr, fcn};
            pull_region(fl, rj, lr, lcn, lc[j], ld[j], kThreads);
        }
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < rj.n * rj.n; idx += kThreads) {
        const int q = Div(rj.n).quot(idx), y = rj.oy + q, x = rj.ox + idx - q * rj.n;
        if (y < dst.rows && x < dst.cols) dst.p[(size_t)y * dst.cols + x] = make_uint2(lc[g][idx], __float_as_uint(ld[g][idx]));
    }
}

// ---- k_remove_apex: one workgroup; `pulled` (at most kRemoveApex samples, its chain at most kRemoveApexChain) to 1 x 1 and back; the
// level with its invalid samples filled goes to `filled`.  The chain's table comes from the host by value: where level k lies in the
// LDS arrays and its size (a level of at most 8192 samples has at most 14 above it); every index into it is uniform.
constexpr int kApexThreads = 1024;
struct ApexChain { int n; int off[16], rows[16], cols[16]; };      // n levels above level 0 = `pulled`

__global__ __launch_bounds__(kApexThreads) void k_remove_apex(Stored pulled, Stored filled, ApexChain t) {
    __shared__ uint32_t C[kRemoveApexChain];
    __shared__ float D[kRemoveApexChain];
    const int n = t.n;
    const int *off = t.off, *lr = t.rows, *lcn = t.cols;
    const int count = lr[0] * lcn[0];
    for (int idx = threadIdx.x; idx < count; idx += kApexThreads) { const uint2 v = pulled.p[idx]; C[idx] = v.x; D[idx] = __uint_as_float(v.y); }
    __syncthreads();
    for (int k = 0; k < n; k++) {
        const int fr = lr[k], fcn = lcn[k], cr = lr[k + 1], ccn = lcn[k + 1];
        const uint32_t *fc = C + off[k]; const float *fd = D + off[k];
        for (int idx = threadIdx.x; idx < cr * ccn; idx += kApexThreads) {
            const int i = idx / ccn, j = idx - i * ccn;
            auto src = [&](int y, int x, uint32_t &c, float &d) {
                if (y >= fr || x >= fcn) return false;
                const uint32_t v = fc[y * fcn + x];
                c = v & 0xffffffu; d = fd[y * fcn + x];
                return (v & kValid) != 0u;
            };
            float d;
            C[off[k + 1] + idx] = pull_sample(src, i, j, d);
            D[off[k + 1] + idx] = d;
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; k--) {
        const int fr = lr[k], fcn = lcn[k], cr = lr[k + 1], ccn = lcn[k + 1];
        for (int idx = threadIdx.x; idx < fr * fcn; idx += kApexThreads) {
            if (C[off[k] + idx] & kValid) continue;
            const int y = idx / fcn, x = idx - y * fcn;
            int yn, yf, xn, xf;
            push_taps(y, cr, yn, yf); push_taps(x, ccn, xn, xf);
            float d;
            const uint32_t out = push_blend(C + off[k + 1], D + off[k + 1], ccn, yn, yf, xn, xf, d);
            if (out) { C[off[k] + idx] = out; D[off[k] + idx] = d; }
        }
        __syncthreads();
    }
    for (int idx = threadIdx.x; idx < count; idx += kApexThreads) filled.p[idx] = make_uint2(C[idx], __float_as_uint(D[idx]));
}

// ---- k_remove_push: the tile's level filled from `coarse`, the FILLED level g above it.  IMAGE: the level is the images and the result
// goes to artistic / depthOut; else the level is `src` (pulled) and the result goes to `out`, the same level filled.
struct Outputs { uint8_t *art; size_t ap; float *z; size_t zp; };

template <bool IMAGE, bool VEC, bool GROW>
__global__ __launch_bounds__(kThreads) void k_remove_push(Images im, Stored src, Stored coarse, Stored out, Outputs o, int rows, int cols, int g) {
    __shared__ TileLds L;
    const int ty = blockIdx.y * kT, tx = blockIdx.x * kT;
    const int lane = threadIdx.x;
    // does the tile hold anything to fill?  IMAGE: a hole needs a selected pixel within `grow` of the tile
    int any = 0;
    if (g > 0) {
        if (IMAGE) {
            const int gr = GROW ? im.grow : 0, W = kT + 2 * gr;
            const Div dw(W);
#pragma unroll 4
            for (int idx = lane; idx < W * W; idx += kThreads) {
                const int i = GROW ? dw.quot(idx) : idx / kT, y = ty - gr + i, x = tx - gr + idx - i * W;
                if (y >= 0 && y < rows && x >= 0 && x < cols) any |= is_selected(im.mask[(size_t)y * im.mp + x], im.select);
            }
        } else {
            for (int idx = lane; idx < kT * kT; idx += kThreads) {
                const int y = ty + idx / kT, x = tx + idx % kT;
                if (y < rows && x < cols) any |= !(src.p[(size_t)y * src.cols + x].x & kValid);
            }
        }
    }
    any = __syncthreads_or(any);                                    // workgroup-uniform from here
    Region r1 = {0, 0, 0};
    int r1rows = 0, r1cols = 0;
    if (any) {
        const Region r0 = {ty - kHalo, tx - kHalo, kR};
        if (IMAGE) classify<kR, GROW>(im, rows, cols, r0.oy, r0.ox, L.selb, L.rowd, L.flags);
        uint32_t *lc[4]; float *ld[4];
        lc[0] = nullptr; lc[1] = L.c1; lc[2] = L.c2; lc[3] = L.c3;
        ld[0] = nullptr; ld[1] = L.d1; ld[2] = L.d2; ld[3] = L.d3;
        Region rj[4];
        int lr[4], lcn[4];
        rj[0] = r0; lr[0] = rows; lcn[0] = cols;
        for (int j = 1; j <= g; j++) { lr[j] = (lr[j - 1] + 1) >> 1; lcn[j] = (lcn[j - 1] + 1) >> 1; rj[j] = {(ty >> j) - (kHalo >> j), (tx >> j) - (kHalo >> j), kR >> j}; }
        // the top of the group: the filled coarse level, a one-sample halo around the tile's part of it
        rj[g] = {(ty >> g) - 1, (tx >> g) - 1, (kT >> g) + 2};
        for (int idx = lane; idx < rj[g].n * rj[g].n; idx += kThreads) {
            const int q = Div(rj[g].n).quot(idx), y = rj[g].oy + q, x = rj[g].ox + idx - q * rj[g].n;
            uint2 v = make_uint2(0u, 0u);
            if (y >= 0 && y < coarse.rows && x >= 0 && x < coarse.cols) v = coarse.p[(size_t)y * coarse.cols + x];
            lc[g][idx] = v.x; ld[g][idx] = __uint_as_float(v.y);
        }
        // the levels between, pulled again
        const FromImages fi = {im, L.flags, r0, rows, cols};
        const FromStored fs = {src};
        for (int j = 1; j < g; j++) {
            if (j == 1) {
                if (IMAGE) pull_region(fi, rj[1], lr[1], lcn[1], lc[1], ld[1], kThreads);
                else pull_region(fs, rj[1], lr[1], lcn[1], lc[1], ld[1], kThreads);
            } else {
                const FromLds fl = {lc[j - 1], ld[j - 1], rj[j - 1], lr[j - 1], lcn[j - 1]};
                pull_region(fl, rj[j], lr[j], lcn[j], lc[j], ld[j], kThreads);
            }
            __syncthreads();
        }
        __syncthreads();
        // and pushed down to the level above the tile's
        for (int j = g - 1; j >= 1; j--) {
            push_region(rj[j], lc[j], ld[j], lr[j], lcn[j], rj[j + 1], lc[j + 1], ld[j + 1], lr[j + 1], lcn[j + 1], kThreads);
            __syncthreads();
        }
        r1 = rj[1]; r1rows = lr[1]; r1cols = lcn[1];
    }
    if (!IMAGE) {
        for (int idx = lane; idx < kT * kT; idx += kThreads) {
            const int y = ty + idx / kT, x = tx + idx % kT;
            if (y >= rows || x >= cols) continue;
            uint2 v = src.p[(size_t)y * src.cols + x];
            if (any && !(v.x & kValid)) {
                float d;
                const uint32_t c = push_sample(L.c1, L.d1, r1, r1rows, r1cols, y, x, d);
                if (c) v = make_uint2(c, __float_as_uint(d));
            }
            out.p[(size_t)y * out.cols + x] = v;
        }
        return;
    }
    // one pixel of the tile from and to memory: o its original as b | g << 8 | r << 16, z its depth; both replaced if it is a filled hole
    auto fill = [&](int y, int x, uint32_t &px, float &z) {
        if (!any || L.flags[(y - ty + kHalo) * kR + (x - tx + kHalo)] != 2) return;
        float d;
        const uint32_t c = push_sample(L.c1, L.d1, r1, r1rows, r1cols, y, x, d);
        if (c) { px = c & 0xffffffu; z = d; }
    };
    auto pixel = [&](int y, int x) {
        uint32_t px = load_bgr(im.orig + (size_t)y * im.op + 3 * (size_t)x);
        float z = *(const float *)((const char *)im.depth + (size_t)y * im.dp + 4 * (size_t)x);
        fill(y, x, px, z);
        store_bgr(o.art + (size_t)y * o.ap + 3 * (size_t)x, px);
        if (o.z) *(float *)((char *)o.z + (size_t)y * o.zp + 4 * (size_t)x) = z;
    };
    if (!VEC) {
        for (int idx = lane; idx < kT * kT; idx += kThreads) {
            const int y = ty + idx / kT, x = tx + idx % kT;
            if (y < rows && x < cols) pixel(y, x);
        }
        return;
    }
    // four pixels per lane: 16 lanes a row of the tile, 16 rows a pass (rows of both images 4-byte, of both depth maps 16-byte aligned)
    for (int pass = 0; pass < kT / 16; pass++) {
        const int y = ty + pass * 16 + (lane >> 4), x = tx + (lane & 15) * 4;
        if (y >= rows || x >= cols) continue;
        if (x + 3 >= cols) { for (int xx = x; xx < cols; xx++) pixel(y, xx); continue; }
        const uint8_t *orow = im.orig + (size_t)y * im.op;
        raw12 v = load_raw<true>(orow, x, cols);
        float4 d4 = *(const float4 *)((const char *)im.depth + (size_t)y * im.dp + 4 * (size_t)x);
        if (any) {
            uint32_t b[12];
            bytes12(v, b);
            float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t px = b[3 * i] | (b[3 * i + 1] << 8) | (b[3 * i + 2] << 16);
                fill(y, x + i, px, dv[i]);
                b[3 * i] = px & 255u; b[3 * i + 1] = (px >> 8) & 255u; b[3 * i + 2] = px >> 16;
            }
            store_bytes12(o.art + (size_t)y * o.ap + 3 * (size_t)x, b);
            d4 = make_float4(dv[0], dv[1], dv[2], dv[3]);
        } else {
            uint32_t *a3 = (uint32_t *)(o.art + (size_t)y * o.ap + 3 * (size_t)x);
            a3[0] = v.w0; a3[1] = v.w1; a3[2] = v.w2;
        }
        if (o.z) *(float4 *)((char *)o.z + (size_t)y * o.zp + 4 * (size_t)x) = d4;
    }
}

// ---- the plan: which levels are stored.  Mirrored by remove_plan() of realtimedepthdiffusion_amd/__init__.py.
struct RemovePlan {
    int groups = 0;                    // P >= 1 pull groups (and as many push groups)
    int g[8] = {};                     // levels each group takes (3; fewer only where the chain ends: an image of at most 4 x 4)
    int rows[9] = {}, cols[9] = {};    // [i]: the level group i reads (0: the image), [groups]: the level the apex takes
    size_t words = 0;                  // of the table buffer: every stored level twice (pulled, filled), 2 words a sample
};

static long long chain_samples(int r, int c) {
    long long n = (long long)r * c;
    while (r > 1 || c > 1) { r = (r + 1) / 2; c = (c + 1) / 2; n += (long long)r * c; }
    return n;
}

static RemovePlan remove_plan(int rows, int cols) {
    RemovePlan p;
    int r = rows, c = cols;
    p.rows[0] = r; p.cols[0] = c;
    do {
        int g = 0;
        while (g < kG && (r > 1 || c > 1)) { r = (r + 1) / 2; c = (c + 1) / 2; g++; }
        p.g[p.groups++] = g;
        p.rows[p.groups] = r; p.cols[p.groups] = c;
        p.words += 4 * (size_t)r * c;
    } while ((long long)r * c > kRemoveApex || chain_samples(r, c) > kRemoveApexChain);
    return p;
}

// rtdd_remove_object (arguments checked by effects_api.cpp): 2 P + 1 launches.
int launch_remove(rtdd_ctx *ctx, const Effect &e) {
    const Effect::Remove &k = e.remove;
    const RemovePlan p = remove_plan(e.rows, e.cols);
    if (const int st = ensure_sat(ctx, p.words)) return st;
    ctx->sat_rows = ctx->sat_cols = 0;                               // whatever table lay here is gone: the next table-path defocus zeroes its padding again
    Stored pulled[9], filled[9];
    uint2 *base = (uint2 *)ctx->sat;
    for (int i = 1; i <= p.groups; i++) {
        const size_t n = (size_t)p.rows[i] * p.cols[i];
        pulled[i] = {base, p.rows[i], p.cols[i]}; filled[i] = {base + n, p.rows[i], p.cols[i]};
        base += 2 * n;
    }
    const Images im = {e.original, e.originalPitch, e.depth, e.depthPitch, k.mask, k.maskPitch, k.removal.select, k.removal.grow, k.removal.sourceMinDepth};
    const Stored none = {nullptr, 0, 0};
    const bool grow = k.removal.grow > 0;
    auto grid = [](int rows, int cols) { return dim3((cols + kT - 1) / kT, (rows + kT - 1) / kT); };
    for (int i = 0; i < p.groups; i++) {
        if (i == 0 && grow) hipLaunchKernelGGL((k_remove_pull<true, true>), grid(p.rows[0], p.cols[0]), dim3(kThreads), 0, ctx->stream, im, none, pulled[1], p.rows[0], p.cols[0], p.g[0]);
        else if (i == 0) hipLaunchKernelGGL((k_remove_pull<true, false>), grid(p.rows[0], p.cols[0]), dim3(kThreads), 0, ctx->stream, im, none, pulled[1], p.rows[0], p.cols[0], p.g[0]);
        else hipLaunchKernelGGL((k_remove_pull<false, false>), grid(p.rows[i], p.cols[i]), dim3(kThreads), 0, ctx->stream, im, pulled[i], pulled[i + 1], p.rows[i], p.cols[i], p.g[i]);
        RTDD_LAUNCH_CHECK(ctx, "k_remove_pull");
    }
    ApexChain chain = {};
    chain.rows[0] = p.rows[p.groups]; chain.cols[0] = p.cols[p.groups];
    while (chain.rows[chain.n] > 1 || chain.cols[chain.n] > 1) {     // (at most 14 steps from 8192 samples; remove_plan bounds the sum)
        const int k = chain.n++;
        chain.off[k + 1] = chain.off[k] + chain.rows[k] * chain.cols[k];
        chain.rows[k + 1] = (chain.rows[k] + 1) / 2; chain.cols[k + 1] = (chain.cols[k] + 1) / 2;
    }
    hipLaunchKernelGGL(k_remove_apex, dim3(1), dim3(kApexThreads), 0, ctx->stream, pulled[p.groups], filled[p.groups], chain);
    RTDD_LAUNCH_CHECK(ctx, "k_remove_apex");
    const Outputs o = {e.artistic, e.artisticPitch, k.depthOut, k.depthOut ? k.depthOutPitch : 0};
    const bool vec = rows_aligned(e.original, e.originalPitch) && rows_aligned(e.artistic, e.artisticPitch) && rows_aligned(e.depth, e.depthPitch, 16) &&
                     (!k.depthOut || rows_aligned(k.depthOut, k.depthOutPitch, 16));
    for (int i = p.groups - 1; i >= 0; i--) {
        const dim3 gr = grid(p.rows[i], p.cols[i]);
#define RTDD_RM_PUSH(V, G) hipLaunchKernelGGL((k_remove_push<true, V, G>), gr, dim3(kThreads), 0, ctx->stream, im, none, filled[1], none, o, p.rows[0], p.cols[0], p.g[0])
        if (i > 0) hipLaunchKernelGGL((k_remove_push<false, false, false>), gr, dim3(kThreads), 0, ctx->stream, im, pulled[i], filled[i + 1], filled[i], o, p.rows[i], p.cols[i], p.g[i]);
        else if (vec) { if (grow) RTDD_RM_PUSH(true, true); else RTDD_RM_PUSH(true, false); }
        else { if (grow) RTDD_RM_PUSH(false, true); else RTDD_RM_PUSH(false, false); }
#undef RTDD_RM_PUSH
        RTDD_LAUNCH_CHECK(ctx, "k_remove_push");
    }
    return RTDD_OK;
}

// ---- k_lift_layer: four texels per lane, a wave 256 texels of a sprite row, a workgroup four rows.  ALIGNED: the sprite's rows are
// 16-byte aligned (one store per lane); else a texel is one dword (4-byte aligned rows) or four bytes.  MATTE (rtdd_lift_layer_matte): the
// mask is an alpha image, select is 0, and a texel's alpha is its byte; the other instantiations are instruction for instruction what
// they were.
template <bool ALIGNED, bool MATTE = false>
__global__ __launch_bounds__(256) void k_lift_layer(const uint8_t *__restrict__ orig, size_t op, const uint8_t *__restrict__ mask, size_t mp, int rows, int cols,
                                                    Effect::Lift k, bool dwords) {
    const int v = blockIdx.y * 4 + wave_id();
    if (v >= k.spriteRows) return;                                   // wave-uniform
    const int u0 = blockIdx.x * 256 + (threadIdx.x & 63) * 4;
    if (u0 >= k.spriteCols) return;
    const int y = k.y + v;
    const bool row_in = y >= 0 && y < rows;
    uint32_t t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = k.x + u0 + i;
        t[i] = 0u;
        if (MATTE) {
            const uint32_t a = row_in && u0 + i < k.spriteCols && x >= 0 && x < cols ? mask[(size_t)y * mp + x] : 0u;
            if (a != 0u) t[i] = load_bgr(orig + (size_t)y * op + 3 * (size_t)x) | (a << 24);
        } else if (row_in && u0 + i < k.spriteCols && x >= 0 && x < cols && is_selected(mask[(size_t)y * mp + x], k.select)) {
            t[i] = load_bgr(orig + (size_t)y * op + 3 * (size_t)x) | 0xff000000u;
        }
    }
    uint8_t *srow = k.sprite + (size_t)v * k.spritePitch + 4 * (size_t)u0;
    if (ALIGNED && u0 + 3 < k.spriteCols) { *(uint4 *)srow = make_uint4(t[0], t[1], t[2], t[3]); return; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (u0 + i >= k.spriteCols) break;
        if (dwords) ((uint32_t *)srow)[i] = t[i];
        else { srow[4 * i] = (uint8_t)t[i]; srow[4 * i + 1] = (uint8_t)(t[i] >> 8); srow[4 * i + 2] = (uint8_t)(t[i] >> 16); srow[4 * i + 3] = (uint8_t)(t[i] >> 24); }
    }
}

// rtdd_lift_layer and rtdd_lift_layer_matte (arguments checked by effects_api.cpp): one launch.
int launch_lift(rtdd_ctx *ctx, const Effect &e) {
    const Effect::Lift &k = e.lift;
    const dim3 g((k.spriteCols + 255) / 256, (k.spriteRows + 3) / 4);
    const bool dwords = rows_aligned(k.sprite, k.spritePitch);
    if (e.kind == Effect::kLiftMatte) {
        if (rows_aligned(k.sprite, k.spritePitch, 16)) hipLaunchKernelGGL((k_lift_layer<true, true>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, k.mask, k.maskPitch, e.rows, e.cols, k, dwords);
        else hipLaunchKernelGGL((k_lift_layer<false, true>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, k.mask, k.maskPitch, e.rows, e.cols, k, dwords);
    } else if (rows_aligned(k.sprite, k.spritePitch, 16)) hipLaunchKernelGGL((k_lift_layer<true>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, k.mask, k.maskPitch, e.rows, e.cols, k, dwords);
    else hipLaunchKernelGGL((k_lift_layer<false>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, k.mask, k.maskPitch, e.rows, e.cols, k, dwords);
    RTDD_LAUNCH_CHECK(ctx, "k_lift_layer");
    return RTDD_OK;
}

}  // namespace rtdd
