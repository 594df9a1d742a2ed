// rtdd_fill_polygon (extension, include/rtdd.h): a closed integer contour filled with a label, a ramp or erased -- the lasso beside the
// brushes of image_kernels.hip.  One launch over the contour's bounding box clipped to the image, in k_paint_strokes' tiles
// (paint_common.hpp).  The vertices travel as kernel arguments (pack_xy: 4 bytes each, 768 at the most: 3 KB, no device buffer, nothing
// of the caller's read after the call returns).
#include <algorithm>

#include "paint_common.hpp"

namespace rtdd {

constexpr int kFillMaxVertices = 768;
struct FillArgs {
    int n;                          // vertices = edges of the closed contour (edge e: v[e] -> v[e + 1 == n ? 0 : e + 1])
    int x0, y0, x1, y1;             // the contour's bounding box clipped to the image (inclusive), x0 rounded down to a multiple of 64
    int evenodd;                    // the rule: covered when w is odd instead of non-zero
    int label0;                     // 0..255, or RTDD_STROKE_ERASE
    int ramp;                       // label0 != label1 on an axis with length: the label rule below; otherwise every covered pixel gets label0
    int ax0, ay0, adx, ady;         // the axis: its first end and its direction
    long long dd, A;                // adx^2 + ady^2;  (2 label0 + 1) dd
    int B;                          // 2 (label1 - label0)
    uint32_t v[kFillMaxVertices];   // pack_xy
};

// a live edge of a tile: cr at the tile's origin, its direction, and the closed box of the boundary test (whose y-range also says whether
// the edge goes up, ya < yb, down or neither)
struct FillEdge { long long cr0; int dxe, dye; int ya_yb, xmin_xmax; };   // the packed pairs: low half | high half << 16, signed halves

// rtdd_paint_ramp_strokes' label rule with the fill's axis as the segment: L = N div D, N = (2 l0 + 1) dd + 2 (l1 - l0) t, t = v.d clamped
// to [0, dd], D = 2 dd.  The axis is the same for every pixel of a launch, so dd, the first term of N (A), the factor of t (B) and
// rcp((float)D) come in ready-made.  A pixel may lie anywhere in the image here, not just in a stroke's grown box: |v| < 2^16 + 2^15,
// |d| < 2^16, so |v.d| < 2^33.2, dd < 2^33, 0 <= N <= 511 dd < 2^42 and D < 2^34 -- inside the bounds ramp_quotient asks for.
__device__ __forceinline__ int fill_label(int px, int py, const FillArgs &C, float rcpD) {
    const long long vx = px - C.ax0, vy = py - C.ay0;
    const long long t = min(max(vx * C.adx + vy * C.ady, 0ll), C.dd);
    const long long N = C.A + (long long)C.B * t;
    return ramp_quotient(N, 2 * C.dd, ramp_f32(N) * rcpD);
}

// The winding number of include/rtdd.h counts, for pixel p, the edges that cross p's row strictly to the RIGHT of p (cr > 0 on an edge
// going up, cr < 0 on one going down: both say "the edge's x on this row exceeds px").  So against a tile an edge is one of three things:
//   nothing: its half-open y-range misses the tile's rows, or it lies wholly left of the tile;
//   base:    wholly right of the tile -- it counts for EVERY pixel of each tile row in its half-open y-range: +-1 on that row's base
//            winding (16 LDS words, accumulated once per tile);
//   live:    its closed box meets the tile (the boundary test's box: an edge that only touches the tile still owns pixels there).
// Live edges are compacted into LDS (a ballot per wave and pass; a sum does not care for their order, so a wave takes its slots from one
// counter) and every pixel walks them.  A tile without a live edge has one winding per row: nothing stored where no row is covered,
// whole rows written without an edge test otherwise -- the inside of a large region costs what a fill costs.
// Per pixel and live edge: cr is affine in the pixel, cr = cr0 + dxe (py - ty0) - dye (px - tx0); cr0 is formed once, in 64 bits, by the
// culling thread (|dxe|, |dye| < 2^16, |origin - a| < 2^16 + 2^15: below 2^34); the pixel's part fits 32 bits (offsets below 64 and 16:
// below 2^22 + 2^20), so the inner loop has no 64-bit multiply, only the sign and the zero of a 64-bit sum.  The record is read at one
// address per wave (an LDS broadcast), and once for the wave's four rows.
__global__ __launch_bounds__(256) void k_fill_polygon(const FillArgs C, uint8_t *__restrict__ edited, size_t editedPitch,
                                                      uint8_t *__restrict__ scribble, size_t scribblePitch,
                                                      const uint8_t *__restrict__ original, size_t originalPitch) {
    __shared__ FillEdge live[kFillMaxVertices];
    __shared__ int base[kPaintTileH];
    __shared__ int total_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int tx0 = C.x0 + (int)blockIdx.x * kPaintTileW, ty0 = C.y0 + (int)blockIdx.y * kPaintTileH;
    const int tx1 = min(tx0 + kPaintTileW - 1, C.x1), ty1 = min(ty0 + kPaintTileH - 1, C.y1);
    if (tid < kPaintTileH) base[tid] = 0;
    if (tid == 0) total_s = 0;
    __syncthreads();
    // cull: edges tid, tid + 256, tid + 512 against this tile (the loop's trip count is the same in every thread: ballots inside)
    for (int first = 0; first < C.n; first += 256) {
        const int e = first + tid;
        bool keep = false;
        FillEdge rec{};
        if (e < C.n) {
            const uint32_t pa = C.v[e], pb = C.v[e + 1 == C.n ? 0 : e + 1];
            const int ax = unpack_x(pa), ay = unpack_y(pa), bx = unpack_x(pb), by = unpack_y(pb);
            const int xmin = min(ax, bx), xmax = max(ax, bx), ymin = min(ay, by), ymax = max(ay, by);
            if (ymin <= ty1 && ymax >= ty0 && xmax >= tx0) {
                if (xmin <= tx1) {
                    keep = true;
                    rec.dxe = bx - ax; rec.dye = by - ay;
                    rec.cr0 = (long long)rec.dxe * (ty0 - ay) - (long long)(tx0 - ax) * rec.dye;
                    rec.ya_yb = (int)((pa >> 16) | (pb & 0xFFFF0000u));
                    rec.xmin_xmax = (int)(((uint32_t)xmin & 0xFFFFu) | ((uint32_t)xmax << 16));
                } else if (ay != by) {
                    const int s = by > ay ? 1 : -1;
                    for (int y = max(ymin, ty0); y <= min(ymax - 1, ty1); y++) atomicAdd(&base[y - ty0], s);
                }
            }
        }
        const unsigned long long mask = __ballot(keep);
        int slot = 0;
        if (lane == 0 && mask) slot = atomicAdd(&total_s, __popcll(mask));
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (keep) live[slot + __popcll(mask & ((1ull << lane) - 1))] = rec;
    }
    __syncthreads();
    const int total = total_s;
    const int x = tx0 + lane, rx = lane;
    if (x > tx1) return;
    const float rcpD = C.ramp ? __builtin_amdgcn_rcpf((float)(unsigned long long)(2 * C.dd)) : 0.0f;
    int w[4];
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { w[k] = base[wave + 4 * k]; on[k] = false; }
    for (int i = 0; i < total; i++) {
        const FillEdge r = live[i];                                  // (one address for the whole wave: an LDS broadcast)
        const int ya = unpack_x(r.ya_yb), yb = r.ya_yb >> 16, xmin = unpack_x(r.xmin_xmax), xmax = r.xmin_xmax >> 16;      // (signed words: the high halves by a shift)
        const bool inx = x >= xmin && x <= xmax;
        long long cr = r.cr0 + (long long)(r.dxe * wave - r.dye * rx);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int y = ty0 + wave + 4 * k;                        // (the same in every lane: the row tests below are the wave's)
            if (ya <= y && y < yb) w[k] += (int)(cr > 0);
            if (yb <= y && y < ya) w[k] -= (int)(cr < 0);
            if (min(ya, yb) <= y && y <= max(ya, yb)) on[k] = on[k] || (cr == 0 && inx);
            cr += (long long)(4 * r.dxe);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int y = ty0 + wave + 4 * k;
        if (y > ty1) break;
        if (!(on[k] || (C.evenodd ? (w[k] & 1) != 0 : w[k] != 0))) continue;
        uint8_t *e = edited + (size_t)y * editedPitch + 3 * x;
        if (C.label0 >= 0) {
            const int label = C.ramp ? fill_label(x, y, C, rcpD) : C.label0;
            e[0] = (uint8_t)label; e[1] = (uint8_t)label; e[2] = (uint8_t)label;
            scribble[(size_t)y * scribblePitch + x] = 255;
        } else {
            const uint8_t *o = original + (size_t)y * originalPitch + 3 * x;
            e[0] = o[0]; e[1] = o[1]; e[2] = o[2];
            scribble[(size_t)y * scribblePitch + x] = 0;
        }
    }
}

// checked by rtdd_fill_polygon (image_api.cpp): 1 <= n <= 768, every coordinate in [-32768, 32767], the rule and the labels valid
int launch_fill_polygon(rtdd_ctx *ctx, const int *xy, int n, const rtdd_fill &fill, const PaintTarget &t) {
    FillArgs C{};
    C.x0 = C.x1 = xy[0]; C.y0 = C.y1 = xy[1];
    for (int i = 0; i < n; i++) {
        const int x = xy[2 * i], y = xy[2 * i + 1];
        C.x0 = std::min(C.x0, x); C.x1 = std::max(C.x1, x); C.y0 = std::min(C.y0, y); C.y1 = std::max(C.y1, y);
        C.v[i] = pack_xy(x, y);
    }
    dim3 grid;
    if (!paint_grid(C.x0, C.y0, C.x1, C.y1, t.rows, t.cols, grid)) return RTDD_OK;      // the contour lies wholly outside the image
    C.n = n;
    C.evenodd = fill.rule == RTDD_FILL_EVEN_ODD;
    C.label0 = fill.label0;
    C.ax0 = fill.ax0; C.ay0 = fill.ay0; C.adx = fill.ax1 - fill.ax0; C.ady = fill.ay1 - fill.ay0;
    C.dd = (long long)C.adx * C.adx + (long long)C.ady * C.ady;
    C.ramp = fill.label0 >= 0 && fill.label0 != fill.label1 && C.dd != 0;
    C.A = (long long)(2 * fill.label0 + 1) * C.dd;
    C.B = 2 * (fill.label1 - fill.label0);
    hipLaunchKernelGGL(k_fill_polygon, grid, dim3(256), 0, ctx->stream, C, t.edited, t.editedPitch, t.scribble, t.scribblePitch, t.original, t.originalPitch);
    RTDD_LAUNCH_CHECK(ctx, "k_fill_polygon");
    return RTDD_OK;
}

}  // namespace rtdd
