// rtdd_segment_surfaces (extension, include/rtdd.h): every connected component of rtdd_fill_surface's link graph at once -- a union-find
// over the H / V link planes, merged by minimum, so that the final parent of every pixel is the smallest linear index y * cols + x of its
// component.  The result is a property of an undirected graph: no schedule changes a byte of it.
//
// In the context's table buffer (ctx->sat): three bit planes laid out as fill_similar.hip's (one 64-bit word per 64 pixels of a row),
//   H, V       rtdd_fill_surface's links (k_surface_links' comparisons, the band given by value)
//   A          the admissible pixels: a pixel of A without a link is a component of one
// then the counters and the candidate list, the parent array P (one int32 per pixel, rows * cols of them, no padding; -1: inadmissible) and
// seven words of record per pixel (field by field: seg_field), used only at the index of a tile-local root.
//
// Six launches (five without a pair to paint), none of them in a loop; one stream synchronisation, two when more than kSegHead
// components have minPixels pixels:
//   k_segment_links     the three planes; the counters zeroed
//   k_segment_local     a 64 x 16 tile (kPaintTileW x kPaintTileH) labelled in LDS: a row's runs of H links are labelled by bit arithmetic
//                       (seg_run_start), the V links inside the tile are united on the LDS labels; P = the tile-local root's index; the
//                       record of every tile-local root cleared (only those can become roots: a component's smallest index is the
//                       smallest index of its part of the tile that holds it)
//   k_segment_merge     the links that cross a tile's bottom and right border, united on P with atomicMin
//   k_segment_flatten   P = the root, the label map; size, box and depth range reduced in LDS per tile-local component, then seven
//                       atomics per tile and local component on the root's record -- never one per pixel or per run
//   k_segment_collect   the roots counted, those of at least minPixels pixels appended to the candidate list (one atomic per workgroup
//                       and counter); the list's order is the schedule's, the host's ranking does not depend on it
//   (host)              counters and the first kSegHead candidates read back in ONE copy (the rest in a second if there are more); the
//                       ranking; the K roots, sorted, and their codes as kernel arguments
//   k_segment_paint     k_wand_paint's tile; the code found under the pixel's root by bisection of the K roots
//
// The union (seg_unite, on LDS labels and on P alike).  Invariants: P[i] <= i; P[i] only ever decreases; P[i] is a pixel of i's component.
// A root is an i with P[i] == i.  unite(a, b): find both roots; equal: done; else atomicMin(P[larger], smaller).  If the word still held
// `larger` the two trees are one.  If it held `old` < larger (another wave linked it meanwhile), the word now holds min(old, smaller):
// larger hangs under one of the two and what is left to do is unite(old, smaller).
// No wave waits for another: there is no flag and no spinning on a value somebody else must write.  Every loop is lock-free and bounded:
// a find walks strictly downwards in index; an iteration of unite that does not return has seen a word that another wave decreased
// since this wave last looked, or walks strictly downwards itself, and the words are bounded below by 0: the sum of all words of P
// strictly decreases with every successful atomicMin, so at most sum(i) iterations fail in all.
// A stale read is safe: whatever old value of P[i] a find reads is a pixel of i's component with an index no larger than i, from which the
// walk goes on downwards; it can cost further steps, never leave the component.  A find that ends at a stale root is caught by the atomic,
// which returns the word's true value.  When the launch has ended every link has been united, so every component is ONE tree whose root
// is its smallest index (its smallest index m has P[m] <= m inside the component: P[m] == m).
// Which unions are skipped: the V link at column x of a word when the V link at x - 1 and both H links (x - 1) - x above and below it are set
// (the two runs are united by the pair to the left); likewise the H link across a word border at row y when the one at y - 1 and the two
// V links under its ends are set.  A skipped union depends only on unions further left or further up, so the dependence is well-founded.
#include <algorithm>
#include <climits>
#include <cstring>
#include <utility>
#include <vector>

#include "effect_common.hpp"
#include "paint_common.hpp"

namespace rtdd {

constexpr int kSegStrip = 8;              // k_surface_links' strip: consecutive rows of one word's columns that a wave walks
constexpr int kSegTile = kPaintTileW * kPaintTileH;
constexpr int kSegHead = 1024;            // candidate records read back with the counters; more than that: a second copy
constexpr int kSegRec = 8;                // words of a candidate's record in the list: the seven fields and the root
enum { kSegPixels = 0, kSegX0, kSegY0, kSegX1, kSegY1, kSegDmin, kSegDmax, kSegRoot };
enum { kSegComponents = 0, kSegCandidates, kSegCounters = 8 };
__host__ __device__ inline int seg_init(int k) { return k == kSegX0 || k == kSegY0 || k == kSegDmin ? INT_MAX : k == kSegPixels ? 0 : -1; }
static_assert(kPaintTileW == 64 && kPaintTileH == 16, "a tile is one word wide and four rows per wave high");
// The records are kept field by field, n = rows * cols words each: the seven words of one root then lie on seven cache lines.  Every tile
// that holds a part of a component adds to that component's seven words; as one 32-byte record they were ONE line, and the 14 000 atomics
// of a component that covers 1080p ran one after the other (k_segment_flatten 165 us; profiles/r26_segment.txt has both).
template <class T> __device__ __forceinline__ T *seg_field(T *rec, size_t n, int f) { return rec + (size_t)f * n; }

// One wave per word and strip, as k_surface_links; lo <= hi are the band itself.  Nothing is read outside the image.
__global__ __launch_bounds__(256) void k_segment_links(const float *__restrict__ depth, size_t depthPitch, int rows, int cols, int W, float step, float lo,
                                                       float hi, u64 *__restrict__ H, u64 *__restrict__ V, u64 *__restrict__ A, int *__restrict__ counters) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kSegCounters) counters[threadIdx.x] = 0;
    const int y0 = ((int)blockIdx.y * 4 + wave_id()) * kSegStrip;
    if (y0 >= rows) return;                                          // wave-uniform: the ballots below have their whole wave
    const int lane = threadIdx.x & 63, x = (int)blockIdx.x * 64 + lane;
    auto at = [&](int yy, int xx) { return remove_depth(((const float *)((const char *)depth + (size_t)yy * depthPitch))[xx]); };
    const bool inx = x < cols, right_in = x + 1 < cols;
    float cur = inx ? at(y0, x) : 0.0f;
    for (int k = 0; k < kSegStrip; k++) {
        const int y = y0 + k;
        if (y >= rows) break;                                        // wave-uniform
        const bool down_in = y + 1 < rows;
        float right = __shfl_down(cur, 1);
        if (lane == 63) right = right_in ? at(y, x + 1) : 0.0f;
        const float down = inx && down_in ? at(y + 1, x) : 0.0f;
        const bool a = inx && lo <= cur && cur <= hi;
        const u64 aw = __ballot(a);
        const u64 hw = __ballot(a && right_in && lo <= right && right <= hi && fabsf(cur - right) <= step);
        const u64 vw = __ballot(a && down_in && lo <= down && down <= hi && fabsf(cur - down) <= step);
        if (lane == 0) {
            const size_t i = (size_t)y * W + blockIdx.x;
            H[i] = hw; V[i] = vw; A[i] = aw;
        }
        cur = down;
    }
}

// the first pixel of the run of H links that holds pixel `lane` of a word: one above the highest missing link below it
__device__ __forceinline__ int seg_run_start(u64 h, int lane) {
    const u64 m = ~h & ((1ull << lane) - 1);
    return m ? 64 - __clzll((long long)m) : 0;
}
// the V links whose union the pair to their left implies: bit x where v, h and the h of the row below are all set at x - 1
__device__ __forceinline__ u64 seg_implied(u64 v, u64 h, u64 hbelow) { return (v & h & hbelow) << 1; }

// LDS labels are read through a volatile pointer, P through relaxed atomic loads: neither may be kept in a register across a loop
struct SegLds {
    int *L;
    __device__ int load(int i) const { return ((volatile int *)L)[i]; }
    __device__ int amin(int i, int v) const { return atomicMin(&L[i], v); }
};
struct SegGlobal {
    int *P;
    __device__ int load(int i) const { return __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int amin(int i, int v) const { return atomicMin(&P[i], v); }
};
template <class M>
__device__ __forceinline__ int seg_find(const M &m, int i) {
    for (int p; (p = m.load(i)) != i; i = p) {}                      // (strictly downwards: p < i)
    return i;
}
template <class M>
__device__ __forceinline__ void seg_unite(const M &m, int a, int b) {
    for (;;) {
        a = seg_find(m, a); b = seg_find(m, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = m.amin(a, b);
        if (old == a) return;
        a = old;                                                     // (old < a: somebody linked a meanwhile)
    }
}

// One tile per workgroup; wave w has the tile's rows w, w + 4, w + 8, w + 12, lane = column.
__global__ __launch_bounds__(256) void k_segment_local(const u64 *__restrict__ H, const u64 *__restrict__ V, const u64 *__restrict__ A, int rows, int cols, int W,
                                                       int *__restrict__ P, int *__restrict__ rec) {
    __shared__ int L[kSegTile];
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int bx = blockIdx.x, ty0 = (int)blockIdx.y * kPaintTileH, x = bx * 64 + lane;
    const SegLds m{L};
    const size_t n = (size_t)rows * cols;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = wave + 4 * k, y = ty0 + r;
        int label = -1;
        if (y < rows) {
            const size_t i = (size_t)y * W + bx;
            if ((A[i] >> lane) & 1) label = r * 64 + seg_run_start(H[i], lane);
        }
        L[r * 64 + lane] = label;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = wave + 4 * k, y = ty0 + r;
        if (r + 1 >= kPaintTileH || y + 1 >= rows) continue;         // (the tile's last row: k_segment_merge's)
        const size_t i = (size_t)y * W + bx;
        const u64 v = V[i];
        if (((v & ~seg_implied(v, H[i], H[i + W])) >> lane) & 1) seg_unite(m, r * 64 + lane, (r + 1) * 64 + lane);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = wave + 4 * k, y = ty0 + r, li = r * 64 + lane;
        if (y >= rows || x >= cols) continue;
        int g = -1;
        if (L[li] >= 0) {
            const int root = seg_find(m, li);
            g = (ty0 + (root >> 6)) * cols + bx * 64 + (root & 63);
            if (root == li) {
#pragma unroll
                for (int f = 0; f < kSegRoot; f++) seg_field(rec, n, f)[g] = seg_init(f);
            }
        }
        P[(size_t)y * cols + x] = g;
    }
}

// One wave per tile: the V links under the tile's last row, then the H links out of its last column.
__global__ __launch_bounds__(64) void k_segment_merge(const u64 *__restrict__ H, const u64 *__restrict__ V, int rows, int cols, int W, int *P) {
    const int lane = threadIdx.x, bx = blockIdx.x, ty0 = (int)blockIdx.y * kPaintTileH;
    const SegGlobal m{P};
    const int yb = ty0 + kPaintTileH - 1;
    if (yb + 1 < rows) {
        const size_t i = (size_t)yb * W + bx;
        const u64 v = V[i];
        if (((v & ~seg_implied(v, H[i], H[i + W])) >> lane) & 1) {   // (a V bit lies below `cols`, in a row that has one below it)
            const int p = yb * cols + bx * 64 + lane;
            seg_unite(m, p, p + cols);
        }
    }
    const int y = ty0 + lane;
    if (bx + 1 < W && lane < kPaintTileH && y < rows) {
        const size_t i = (size_t)y * W + bx;
        if (H[i] >> 63) {                                            // (set only where column 64 bx + 64 lies inside the image)
            const bool implied = y > 0 && (H[i - W] >> 63) && (V[i - W] >> 63) && (V[i - W + 1] & 1);
            if (!implied) {
                const int p = y * cols + bx * 64 + 63;
                seg_unite(m, p, p + 1);
            }
        }
    }
}

// One tile per workgroup, as k_segment_local.  A pixel's slot is the tile-local position of the parent k_segment_local gave it where that
// still lies in the tile, its own otherwise: all pixels of a slot have one root.  A row of a wave that lies in one slot (the usual case)
// is reduced in registers and costs seven LDS atomics, not 7 x 64.
__global__ __launch_bounds__(256) void k_segment_flatten(const float *__restrict__ depth, size_t depthPitch, int rows, int cols, int *P, int *__restrict__ rec,
                                                         int32_t *__restrict__ labels, size_t labelsPitch) {
    __shared__ int acc[kSegRec][kSegTile];                           // [kSegRoot]: the slot's root
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int bx = blockIdx.x, ty0 = (int)blockIdx.y * kPaintTileH, x = bx * 64 + lane;
    const SegGlobal m{P};
    const size_t n = (size_t)rows * cols;
    for (int i = threadIdx.x; i < kSegRec * kSegTile; i += 256) acc[i / kSegTile][i % kSegTile] = seg_init(i / kSegTile);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = wave + 4 * k, y = ty0 + r;
        if (y >= rows) break;                                        // wave-uniform
        int q = -1, root = -1, slot = r * 64 + lane, dbits = 0;
        if (x < cols) {
            const size_t p = (size_t)y * cols + x;
            q = P[p];
            if (q >= 0) {
                root = seg_find(m, q);
                if (root != q) P[p] = root;
                const int qy = q / cols - ty0, qx = q % cols - bx * 64;
                if (qy >= 0 && qy < kPaintTileH && qx >= 0 && qx < 64) slot = qy * 64 + qx;
                dbits = __float_as_int(remove_depth(((const float *)((const char *)depth + (size_t)y * depthPitch))[x]));
            }
            if (labels) ((int32_t *)((char *)labels + (size_t)y * labelsPitch))[x] = root;
        }
        const bool in = root >= 0;
        const u64 mask = __ballot(in);
        if (mask == 0) continue;                                     // wave-uniform
        const int first = __ffsll((unsigned long long)mask) - 1;
        const int slot0 = __shfl(slot, first);
        if (__ballot(in && slot != slot0) == 0) {
            int lo = in ? dbits : INT_MAX, hi = in ? dbits : -1;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) { lo = min(lo, __shfl_xor(lo, s)); hi = max(hi, __shfl_xor(hi, s)); }
            if (lane == first) {
                atomicAdd(&acc[kSegPixels][slot0], __popcll(mask));
                atomicMin(&acc[kSegX0][slot0], bx * 64 + first); atomicMax(&acc[kSegX1][slot0], bx * 64 + 63 - __clzll((long long)mask));
                atomicMin(&acc[kSegY0][slot0], y); atomicMax(&acc[kSegY1][slot0], y);
                atomicMin(&acc[kSegDmin][slot0], lo); atomicMax(&acc[kSegDmax][slot0], hi);
                acc[kSegRoot][slot0] = root;                         // (every writer of a slot writes the same root)
            }
        } else if (in) {
            atomicAdd(&acc[kSegPixels][slot], 1);
            atomicMin(&acc[kSegX0][slot], x); atomicMax(&acc[kSegX1][slot], x);
            atomicMin(&acc[kSegY0][slot], y); atomicMax(&acc[kSegY1][slot], y);
            atomicMin(&acc[kSegDmin][slot], dbits); atomicMax(&acc[kSegDmax][slot], dbits);
            acc[kSegRoot][slot] = root;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kSegTile; s += 256) {
        if (acc[kSegPixels][s] == 0) continue;
        const int root = acc[kSegRoot][s];                           // (a root's record: cleared by k_segment_local)
        atomicAdd(&seg_field(rec, n, kSegPixels)[root], acc[kSegPixels][s]);
        atomicMin(&seg_field(rec, n, kSegX0)[root], acc[kSegX0][s]); atomicMin(&seg_field(rec, n, kSegY0)[root], acc[kSegY0][s]);
        atomicMax(&seg_field(rec, n, kSegX1)[root], acc[kSegX1][s]); atomicMax(&seg_field(rec, n, kSegY1)[root], acc[kSegY1][s]);
        atomicMin(&seg_field(rec, n, kSegDmin)[root], acc[kSegDmin][s]); atomicMax(&seg_field(rec, n, kSegDmax)[root], acc[kSegDmax][s]);
    }
}

// One thread per pixel, in linear order.  At most n / minPixels components have minPixels pixels: the list cannot overflow.
__global__ __launch_bounds__(256) void k_segment_collect(const int *__restrict__ P, const int *__restrict__ rec, int n, int minPixels, int most, int *__restrict__ counters,
                                                         int *__restrict__ list) {
    __shared__ int roots[4], cands[4], base;
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;         // (n <= 2^30)
    const bool root = i < n && P[i] == i;
    const bool cand = root && seg_field(rec, (size_t)n, kSegPixels)[i] >= minPixels;
    const u64 rmask = __ballot(root), cmask = __ballot(cand);
    if (lane == 0) { roots[wave] = __popcll(rmask); cands[wave] = __popcll(cmask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nr = roots[0] + roots[1] + roots[2] + roots[3], nc = cands[0] + cands[1] + cands[2] + cands[3];
        if (nr) atomicAdd(&counters[kSegComponents], nr);
        base = nc ? atomicAdd(&counters[kSegCandidates], nc) : 0;
    }
    __syncthreads();
    if (!cand) return;
    int at = base + __popcll(cmask & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) at += cands[w];
    if (at >= most) return;                                          // (cannot happen: the sizes add up to at most n; the host checks the counter)
    int *o = list + (size_t)at * kSegRec;
#pragma unroll
    for (int f = 0; f < kSegRoot; f++) o[f] = seg_field(rec, (size_t)n, f)[i];
    o[kSegRoot] = i;
}

struct SegTable { int n; int roots[255]; uint8_t codes[256]; };     // roots ascending, codes[k] the code of roots[k]

// k_wand_paint's tile and write; x0 = y0 = 0: the launch covers the image
__global__ __launch_bounds__(256) void k_segment_paint(const SegTable T, const int *__restrict__ P, int rows, int cols, uint8_t *__restrict__ edited,
                                                       size_t editedPitch, uint8_t *__restrict__ scribble, size_t scribblePitch) {
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int x = (int)blockIdx.x * kPaintTileW + lane, ty0 = (int)blockIdx.y * kPaintTileH;
    if (x >= cols) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int y = ty0 + wave + 4 * k;
        if (y >= rows) break;
        const int root = P[(size_t)y * cols + x];
        if (root < 0) continue;
        int a = 0, b = T.n;                                          // the first index whose root is not below the pixel's
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (T.roots[mid] < root) a = mid + 1; else b = mid;
        }
        if (a == T.n || T.roots[a] != root) continue;
        const uint8_t code = T.codes[a];
        uint8_t *e = edited + (size_t)y * editedPitch + 3 * x;
        e[0] = code; e[1] = code; e[2] = code;
        scribble[(size_t)y * scribblePitch + x] = 255;
    }
}

// checked by rtdd_segment_surfaces (image_api.cpp).  t.edited and t.scribble are both null or both given.  SYNCHRONISES once, or twice;
// the paint pass is queued behind the last synchronisation.
int launch_segment_surfaces(rtdd_ctx *ctx, const rtdd_segmentation &sg, const PaintTarget &t, const float *depth, size_t depthPitch, int32_t *labels,
                            size_t labelsPitch, rtdd_segment *segments, rtdd_segment_info *out) {
    const int rows = t.rows, cols = t.cols, W = (cols + 63) / 64, tilesY = (rows + kPaintTileH - 1) / kPaintTileH;
    const size_t plane = (size_t)rows * W, n = (size_t)rows * cols, most = n / (size_t)sg.minPixels;
    const size_t words = 6 * plane + kSegCounters + kSegRec * most + n + kSegRoot * n;
    if (ensure_sat(ctx, words) != RTDD_OK) {
        (void)hipGetLastError();
        return fail(ctx, RTDD_ERR_NOMEM, "segment_surfaces: the planes, the parents and the records could not be allocated");
    }
    ctx->sat_rows = ctx->sat_cols = 0;                               // (as launch_fill_similar)
    u64 *H = (u64 *)ctx->sat, *V = H + plane, *A = V + plane;
    int *counters = (int *)(A + plane), *list = counters + kSegCounters, *P = list + kSegRec * most, *rec = P + n;
    const dim3 tiles(W, tilesY);
    hipLaunchKernelGGL(k_segment_links, dim3(W, (rows + 4 * kSegStrip - 1) / (4 * kSegStrip)), dim3(256), 0, ctx->stream, depth, depthPitch, rows, cols, W,
                       sg.step, sg.lo, sg.hi, H, V, A, counters);
    RTDD_LAUNCH_CHECK(ctx, "k_segment_links");
    hipLaunchKernelGGL(k_segment_local, tiles, dim3(256), 0, ctx->stream, H, V, A, rows, cols, W, P, rec);
    RTDD_LAUNCH_CHECK(ctx, "k_segment_local");
    hipLaunchKernelGGL(k_segment_merge, tiles, dim3(64), 0, ctx->stream, H, V, rows, cols, W, P);
    RTDD_LAUNCH_CHECK(ctx, "k_segment_merge");
    hipLaunchKernelGGL(k_segment_flatten, tiles, dim3(256), 0, ctx->stream, depth, depthPitch, rows, cols, P, rec, labels, labelsPitch);
    RTDD_LAUNCH_CHECK(ctx, "k_segment_flatten");
    hipLaunchKernelGGL(k_segment_collect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, P, rec, (int)n, sg.minPixels, (int)most, counters, list);
    RTDD_LAUNCH_CHECK(ctx, "k_segment_collect");
    const size_t head = std::min<size_t>(kSegHead, most);
    std::vector<int> host(kSegCounters + kSegRec * head);
    RTDD_HIP(ctx, hipMemcpyAsync(host.data(), counters, host.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int components = host[kSegComponents], candidates = host[kSegCandidates];
    if ((size_t)candidates > most) return fail(ctx, RTDD_ERR_STATE, "segment_surfaces: more candidates than rows * cols / minPixels (cannot happen)");
    if ((size_t)candidates > head) {
        host.resize(kSegCounters + kSegRec * (size_t)candidates);
        RTDD_HIP(ctx, hipMemcpyAsync(host.data() + kSegCounters, list, kSegRec * (size_t)candidates * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the ranking: size descending, then root ascending
    std::vector<const int *> order((size_t)candidates);
    for (int i = 0; i < candidates; i++) order[i] = host.data() + kSegCounters + kSegRec * (size_t)i;
    const int K = std::min(candidates, sg.maxRegions);
    std::partial_sort(order.begin(), order.begin() + K, order.end(), [](const int *a, const int *b) {
        return a[kSegPixels] != b[kSegPixels] ? a[kSegPixels] > b[kSegPixels] : a[kSegRoot] < b[kSegRoot];
    });
    long long pixels = 0;
    for (int k = 0; k < K; k++) {
        const int *q = order[k];
        pixels += q[kSegPixels];
        if (segments) {
            rtdd_segment &s = segments[k];
            s.code = sg.firstCode + k; s.pixels = q[kSegPixels];
            s.rootX = q[kSegRoot] % cols; s.rootY = q[kSegRoot] / cols;
            s.x0 = q[kSegX0]; s.y0 = q[kSegY0]; s.x1 = q[kSegX1]; s.y1 = q[kSegY1];
            static_assert(sizeof(float) == sizeof(int), "the depth range travels as bits");
            memcpy(&s.dmin, &q[kSegDmin], sizeof(float)); memcpy(&s.dmax, &q[kSegDmax], sizeof(float));
        }
    }
    if (out) *out = rtdd_segment_info{components, candidates, K, (int)pixels};
    if (t.edited && K > 0) {
        std::vector<std::pair<int, int>> byRoot((size_t)K);
        for (int k = 0; k < K; k++) byRoot[k] = {order[k][kSegRoot], sg.firstCode + k};
        std::sort(byRoot.begin(), byRoot.end());
        SegTable T{};
        T.n = K;
        for (int k = 0; k < K; k++) { T.roots[k] = byRoot[k].first; T.codes[k] = (uint8_t)byRoot[k].second; }
        hipLaunchKernelGGL(k_segment_paint, tiles, dim3(256), 0, ctx->stream, T, P, rows, cols, t.edited, t.editedPitch, t.scribble, t.scribblePitch);
        RTDD_LAUNCH_CHECK(ctx, "k_segment_paint");
    }
    return RTDD_OK;
}

}  // namespace rtdd
