// image_kernels.hip -- the annotation side: the reference's three byte kernels (Dirichlet injection K5, 2x annotation down-sample K6,
// square brush K7: one wave covers 64 consecutive pixels of a row so mask/depth accesses coalesce); the annotation pyramid of an estimate
// in one launch, accumulating or rebuilding, its chain through global memory or in LDS (two kernel templates); brush
// strokes, constant or ramped (k_paint_strokes<>, which shares paint_common.hpp with fill_polygon.hip's lasso); and the row re-pitch
// copy.  All tiny and HBM-latency-bound.  Their launchers follow the kernels.
#include <algorithm>
#include <type_traits>

#include "paint_common.hpp"

namespace rtdd {

// convert (K5) -- src/GPUImageProcessing.cu:8-21
__global__ __launch_bounds__(256) void k_convert(const uint8_t *__restrict__ src, size_t srcPitch, float *__restrict__ dst, size_t dstPitch,
                                                 const uint8_t *__restrict__ mask, size_t maskPitch, int rows, int cols, size_t zSrc, size_t zDst, size_t zMask) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + wave_id();
    if (x >= cols || y >= rows) return;
    RTDD_Z(src, zSrc); RTDD_Z(dst, zDst); RTDD_Z(mask, zMask);
    if (mask[(size_t)y * maskPitch + x] == 255)
        ((float *)((char *)dst + (size_t)y * dstPitch))[x] = (float)src[(size_t)y * srcPitch + 3 * x];
}

// pyrDown (K6) -- src/GPUImageProcessing.cu:23-49.  Scan order py outer, px inner, later hits
// overwrite earlier ones; nothing is ever cleared; channels 1,2 of the coarse image untouched.
__global__ __launch_bounds__(256) void k_pyrdown_annotation(const uint8_t *__restrict__ ps, size_t psp, const uint8_t *__restrict__ pe, size_t pep,
                                                            int prows, int pcols, uint8_t *__restrict__ cs, size_t csp,
                                                            uint8_t *__restrict__ ce, size_t cep, int crows, int ccols, size_t zPs, size_t zPe, size_t zCs, size_t zCe) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + wave_id();
    if (x >= ccols || y >= crows) return;
    RTDD_Z(ps, zPs); RTDD_Z(pe, zPe); RTDD_Z(cs, zCs); RTDD_Z(ce, zCe);
    int hit = -1;
#pragma unroll
    for (int j = -1; j <= 0; j++)
#pragma unroll
        for (int i = -1; i <= 0; i++) {
            const int px = 2 * x + i, py = 2 * y + j;
            if (px >= 0 && py >= 0 && px < pcols && py < prows && ps[(size_t)py * psp + px] == 255)
                hit = pe[(size_t)py * pep + 3 * px];
        }
    if (hit >= 0) {
        cs[(size_t)y * csp + x] = 255;
        ce[(size_t)y * cep + 3 * x] = (uint8_t)hit;
    }
}

// The whole annotation pyramid of an estimate in ONE launch (src/main.cpp:249-259: P - 1 GPUPyrDownAnnotation calls, then
// GPUConvertToFloat on the coarsest level).  A coarse pixel x looks at the fine pixels 2x - 1 and 2x (above), so the level-l pixels
// [a 2^l - (2^l - 1), a 2^l] and nothing else feed level-(l + k) pixel a ... : the footprints of the coarsest level's pixels tile
// EVERY level disjointly.  A workgroup therefore owns kApB x kApB pixels of the coarsest level and, level by level, all the pixels of the
// finer levels under them: it writes a level, __syncthreads(), and reads it back for the next one -- no other workgroup touches those
// pixels, the scan order and "last hit wins" are pyrDown's above.  Pixels of a fine level beyond the last coarsest pixel's footprint (the
// level sizes are floors) belong to the workgroups of the next tile row / column: the grid is one tile larger than the coarsest level
// needs.  Five launches of ~7 us each (dependent, tiny) -> one: a live 1080p frame 1.18 -> 1.15 ms of GPU time
// (profiles/r05_live_timeline_*).
constexpr int kApMaxLevels = 12, kApB = 2;
struct AnnotationPyramid {
    int levels;                                   // P
    uint8_t *scribble[kApMaxLevels], *edited[kApMaxLevels];
    size_t sp[kApMaxLevels], ep[kApMaxLevels];    // pitches
    size_t zs[kApMaxLevels], ze[kApMaxLevels];    // byte strides between the images of a batch (blockIdx.z)
    int rows[kApMaxLevels], cols[kApMaxLevels];
    float *depth; size_t dp, zd;                  // the coarsest level's depth image (src/main.cpp:257-259)
};

// The chain through global memory (any depth).  kRebuild = false accumulates: the coarse images keep what earlier frames left, exactly
// as with one launch per level.  kRebuild = true (rtdd_pyramid_annotation_rebuild, an erasing paint call) builds the coarse levels as if
// they had been all zero before the down-sampling: the footprints tile every level completely and disjointly, so each workgroup simply
// stores EVERY pixel of its footprint and never reads the old coarse contents -- no memsets in front, one launch.  The store is all that
// differs: accumulating, only on a hit, the flag and channel 0 (K6: nothing is ever cleared); rebuilding, every pixel, hit or not:
// scribble 255 / 0, edited (winner, 0, 0) / (0, 0, 0) -- channels 1 and 2 of a coarse edited image are never written by
// GPUPyrDownAnnotation and are zero after creation.
// (The scan, the footprint origin and the convert tail are written out here and again in the LDS chain: as __forceinline__ functions
// they moved the kernels' scalar loads and address arithmetic, and scripts/effect_isa_diff.py --multiset is the yardstick of this file.)
template <bool kRebuild>
__global__ __launch_bounds__(256) void k_annotation_pyramid(AnnotationPyramid A) {
    const int P = A.levels, top = P - 1;
    const size_t z = blockIdx.z;
    for (int l = 1; l <= top; l++) {
        const int f = 1 << (top - l);                                // level-l pixels per coarsest pixel, per direction
        // this workgroup's pixels of level l: [X0 f - (f - 1), (X0 + kApB - 1) f] x the same in y, clipped to the level
        const int xa = max((int)blockIdx.x * kApB * f - (f - 1), 0), xb = min(((int)blockIdx.x * kApB + kApB - 1) * f, A.cols[l] - 1);
        const int ya = max((int)blockIdx.y * kApB * f - (f - 1), 0), yb = min(((int)blockIdx.y * kApB + kApB - 1) * f, A.rows[l] - 1);
        const int w = xb - xa + 1, h = yb - ya + 1;
        if (w > 0 && h > 0) {
            const uint8_t *ps = A.scribble[l - 1] + z * A.zs[l - 1], *pe = A.edited[l - 1] + z * A.ze[l - 1];
            uint8_t *cs = A.scribble[l] + z * A.zs[l], *ce = A.edited[l] + z * A.ze[l];
            const int prows = A.rows[l - 1], pcols = A.cols[l - 1];
            for (int i = threadIdx.x; i < w * h; i += 256) {
                const int x = xa + i % w, y = ya + i / w;
                int hit = -1;
#pragma unroll
                for (int jj = -1; jj <= 0; jj++)
#pragma unroll
                    for (int ii = -1; ii <= 0; ii++) {
                        const int px = 2 * x + ii, py = 2 * y + jj;
                        if (px >= 0 && py >= 0 && px < pcols && py < prows && ps[(size_t)py * A.sp[l - 1] + px] == 255)
                            hit = pe[(size_t)py * A.ep[l - 1] + 3 * px];
                    }
                if constexpr (kRebuild) {
                    cs[(size_t)y * A.sp[l] + x] = hit >= 0 ? 255 : 0;
                    uint8_t *e = ce + (size_t)y * A.ep[l] + 3 * x;
                    e[0] = (uint8_t)(hit >= 0 ? hit : 0); e[1] = 0; e[2] = 0;
                } else if (hit >= 0) {
                    cs[(size_t)y * A.sp[l] + x] = 255;
                    ce[(size_t)y * A.ep[l] + 3 * x] = (uint8_t)hit;
                }
            }
        }
        __syncthreads();                                             // the level is read back by this workgroup only
    }
    // convert (K5) on the coarsest level: the workgroup's kApB x kApB pixels
    const int x = (int)blockIdx.x * kApB + (int)(threadIdx.x % kApB), y = (int)blockIdx.y * kApB + (int)(threadIdx.x / kApB);
    if (threadIdx.x < kApB * kApB && A.depth && x < A.cols[top] && y < A.rows[top]) {
        const uint8_t *m = A.scribble[top] + z * A.zs[top], *e = A.edited[top] + z * A.ze[top];
        if (m[(size_t)y * A.sp[top] + x] == 255)
            ((float *)((char *)A.depth + z * A.zd + (size_t)y * A.dp))[x] = (float)e[(size_t)y * A.ep[top] + 3 * x];
    }
}

// The same pyramid with the chain in LDS (pyramids of up to six levels: every size up to 4K).  In footprint-local coordinates (origin =
// the unclipped first pixel of the workgroup's footprint on that level) level-l pixel (lx, ly) reads level-(l - 1) pixels
// (2 lx + {0, 1}, 2 ly + {0, 1}), and all a level hands to the next is "the edited value where the scribble flag is 255, else nothing":
// one short per pixel.  Every global load of the workgroup is issued before the first is used (ONE memory round trip; a first version
// that stored each level's map to LDS as it arrived paid one per level and measured no faster than the global chain: EXPERIMENTS.md),
// then the levels are walked in LDS and stored.  Where the two variants differ:
//   the preload    accumulating: the level-0 footprint and, because the coarse images accumulate over the frames, the OLD state of every
//                  coarser level.  Rebuilding: level 0 only, a fifth of the loads (the old coarse state is not wanted), its flag masked
//                  by `in` as it is loaded.
//   the map write  accumulating: only a pixel inside the level that was hit (its old state is in the map already).  Rebuilding: always,
//                  in ? hit : -1 -- a pixel outside the level hands nothing on, as in the global chain.
//   the store      as in the global chain: the pixels that were hit / every pixel of every coarse footprint.
template <int TOP, bool kRebuild>
__global__ __launch_bounds__(256) void k_annotation_pyramid_lds(AnnotationPyramid A) {
    constexpr int kN0 = kApB << TOP, kE0 = (kN0 * kN0 + 255) / 256;  // level-0 footprint edge, its entries per thread
    constexpr int kTotal = (4 * kN0 * kN0 - kApB * kApB) / 3;       // sum over the levels of (kApB << (TOP - l))^2
    constexpr int kLoaded = kRebuild ? 0 : TOP;                      // the last level that is preloaded
    __shared__ short map[kTotal];
    const int tid = threadIdx.x;
    const size_t z = blockIdx.z;
    int flag[kLoaded + 1][kE0], val[kLoaded + 1][kE0];
#pragma unroll
    for (int l = 0; l <= kLoaded; l++) {
        const int f = 1 << (TOP - l), n = kApB * f;
        const int x0 = (int)blockIdx.x * kApB * f - (f - 1), y0 = (int)blockIdx.y * kApB * f - (f - 1);
        const uint8_t *ps = A.scribble[l] + z * A.zs[l], *pe = A.edited[l] + z * A.ze[l];
#pragma unroll
        for (int k = 0; k < kE0; k++) {
            if (k * 256 >= n * n) continue;                          // (compile time after unrolling: the coarser levels have fewer entries)
            const int i = tid + 256 * k, lx = i & (n - 1), ly = i / n, x = x0 + lx, y = y0 + ly;
            const bool in = i < n * n && x >= 0 && y >= 0 && x < A.cols[l] && y < A.rows[l];
            const int xc = in ? x : 0, yc = in ? y : 0;
            if constexpr (kRebuild) flag[l][k] = in ? ps[(size_t)yc * A.sp[l] + xc] : 0;
            else flag[l][k] = ps[(size_t)yc * A.sp[l] + xc];
            val[l][k] = pe[(size_t)yc * A.ep[l] + 3 * xc];
        }
    }
    int off = 0;
#pragma unroll
    for (int l = 0; l <= kLoaded; l++) {
        const int f = 1 << (TOP - l), n = kApB * f;
        const int x0 = (int)blockIdx.x * kApB * f - (f - 1), y0 = (int)blockIdx.y * kApB * f - (f - 1);
#pragma unroll
        for (int k = 0; k < kE0; k++) {
            if (k * 256 >= n * n) continue;
            const int i = tid + 256 * k, lx = i & (n - 1), ly = i / n, x = x0 + lx, y = y0 + ly;
            const bool in = kRebuild || (x >= 0 && y >= 0 && x < A.cols[l] && y < A.rows[l]);
            if (i < n * n) map[off + i] = (short)((in && flag[l][k] == 255) ? val[l][k] : -1);
        }
        off += n * n;
    }
    __syncthreads();
    int poff = 0;
#pragma unroll
    for (int l = 1; l <= TOP; l++) {
        const int f = 1 << (TOP - l), n = kApB * f, pn = 2 * n, coff = poff + pn * pn;
        const int x0 = (int)blockIdx.x * kApB * f - (f - 1), y0 = (int)blockIdx.y * kApB * f - (f - 1);
        uint8_t *cs = A.scribble[l] + z * A.zs[l], *ce = A.edited[l] + z * A.ze[l];
#pragma unroll
        for (int k = 0; k < kE0; k++) {
            if (k * 256 >= n * n) continue;
            const int i = tid + 256 * k;
            if (i < n * n) {
                const int lx = i & (n - 1), ly = i / n, x = x0 + lx, y = y0 + ly;
                const short *q = map + poff + (2 * ly) * pn + 2 * lx;
                int hit = -1;                                        // scan order py outer, px inner, the last hit wins (k_pyrdown_annotation)
                if (q[0] >= 0) hit = q[0];
                if (q[1] >= 0) hit = q[1];
                if (q[pn] >= 0) hit = q[pn];
                if (q[pn + 1] >= 0) hit = q[pn + 1];
                if constexpr (kRebuild) {
                    const bool in = x >= 0 && y >= 0 && x < A.cols[l] && y < A.rows[l];
                    map[coff + i] = (short)(in ? hit : -1);
                    if (in) {
                        cs[(size_t)y * A.sp[l] + x] = hit >= 0 ? 255 : 0;
                        uint8_t *e = ce + (size_t)y * A.ep[l] + 3 * x;
                        e[0] = (uint8_t)(hit >= 0 ? hit : 0); e[1] = 0; e[2] = 0;
                    }
                } else if (hit >= 0 && x >= 0 && y >= 0 && x < A.cols[l] && y < A.rows[l]) {
                    map[coff + i] = (short)hit;
                    cs[(size_t)y * A.sp[l] + x] = 255;
                    ce[(size_t)y * A.ep[l] + 3 * x] = (uint8_t)hit;
                }
            }
        }
        __syncthreads();
        poff = coff;
    }
    // convert (K5) on the coarsest level: the workgroup's kApB x kApB pixels, whose labels the map holds
    const int x = (int)blockIdx.x * kApB + (tid % kApB), y = (int)blockIdx.y * kApB + (tid / kApB);
    if (tid < kApB * kApB && A.depth && x < A.cols[TOP] && y < A.rows[TOP]) {
        const int v = map[poff + tid];
        if (v >= 0) ((float *)((char *)A.depth + z * A.zd + (size_t)y * A.dp))[x] = (float)v;
    }
}

// paintImage (K7) -- src/GPUImageProcessing.cu:51-70.  Launched over the brush's bounding box only
// (the reference launches the whole image and discards all but the brush).
__global__ __launch_bounds__(256) void k_paint(int x0, int y0, int x1, int y1, int color, uint8_t *__restrict__ edited, size_t editedPitch,
                                               uint8_t *__restrict__ scribble, size_t scribblePitch) {
    const int x = x0 + blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = y0 + blockIdx.y * 4 + wave_id();
    if (x > x1 || y > y1) return;
    uint8_t *e = edited + (size_t)y * editedPitch + 3 * x;
    e[0] = (uint8_t)color; e[1] = (uint8_t)color; e[2] = (uint8_t)color;
    scribble[(size_t)y * scribblePitch + x] = 255;
}

// rtdd_paint_strokes (extension, include/rtdd.h): up to kStrokeChunk segments per launch, painted or erased in array order.  The records
// travel as kernel arguments (12 bytes each: no device buffer, no staging area to keep alive, nothing of the caller's read after the call
// returns); a longer array is a sequence of launches, whose stream order is the array's order.  A workgroup owns a 64 x 16 tile of the
// chunk's bounding box (4 pixels per thread, one wave per row as everywhere here): thread i tests stroke i's own bounding box, grown by
// its half-width, against the tile; the survivors are compacted IN ORDER into LDS (a ballot per wave, a four-entry prefix), and every
// pixel walks them from the last to the first and stops at the first that covers it.  All integer, exact on the whole documented domain:
// endpoints in [-32768, 32767], pixels in [0, 32767], radius <= 1024, so inside a stroke's grown box |v| and |d| stay below 2^17, every
// product below 2^35, and the one square that can pass 2^63 -- (2 cross)^2 -- is compared only after 2 |cross| < 2^32 (at or beyond that
// it exceeds radius^2 * |d|^2 <= 2^54 anyway).
constexpr int kStrokeChunk = 256;
struct PackedStroke { uint32_t p0, p1, meta; };  // the two ends (pack_xy); radius | brush << 11 | (label + 1) << 12 [| label1 << 21: a ramp]
struct StrokeChunk {
    int count, x0, y0, x1, y1;                    // strokes in this chunk; its bounding box, clipped to the image (inclusive)
    PackedStroke s[kStrokeChunk];
};

__device__ __forceinline__ bool stroke_covers(int px, int py, uint32_t p0, uint32_t p1, int radius, int brush) {
    const int x0 = unpack_x(p0), y0 = unpack_y(p0), x1 = unpack_x(p1), y1 = unpack_y(p1), h = radius / 2;
    if (px < min(x0, x1) - h || px > max(x0, x1) + h || py < min(y0, y1) - h || py > max(y0, y1) + h) return false;
    const long long dx = x1 - x0, dy = y1 - y0, vx = px - x0, vy = py - y0;
    const long long cross = dx * vy - dy * vx;
    const unsigned long long ac = (unsigned long long)(cross < 0 ? -cross : cross);
    if (brush == RTDD_BRUSH_SQUARE) return ac <= (unsigned long long)h * (unsigned long long)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
    const long long t = vx * dx + vy * dy, dd = dx * dx + dy * dy, r2 = (long long)radius * radius;
    if (t <= 0) return 4 * (vx * vx + vy * vy) <= r2;
    if (t >= dd) { const long long wx = px - x1, wy = py - y1; return 4 * (wx * wx + wy * wy) <= r2; }
    const unsigned long long c2 = 2 * ac;
    return c2 < (1ull << 32) && c2 * c2 <= (unsigned long long)r2 * (unsigned long long)dd;
}

// rtdd_paint_ramp_strokes' label of a covered pixel (include/rtdd.h), for dd != 0: L = N div (2 dd), N = 2 (l0 (dd - t) + l1 t) + dd,
// t = v.d clamped to [0, dd].  N is formed as (2 l0 + 1) dd + 2 (l1 - l0) t: the same integer, its first term the same in every lane.
// Called only behind stroke_covers, i.e. inside the stroke's grown box, where |v|, |d| < 2^17: |v.d| and dd < 2^35, and 0 <= N <=
// 511 dd < 2^45, D = 2 dd < 2^36 -- every product below fits 64 bits with room.
// (ramp_quotient, paint_common.hpp, has the division and its error bound.)
__device__ __forceinline__ int ramp_label(int px, int py, uint32_t p0, uint32_t p1, int l0, int l1) {
    const int x0 = unpack_x(p0), y0 = unpack_y(p0), x1 = unpack_x(p1), y1 = unpack_y(p1);
    const long long dx = x1 - x0, dy = y1 - y0, vx = px - x0, vy = py - y0, dd = dx * dx + dy * dy;
    const long long t = min(max(vx * dx + vy * dy, 0ll), dd);
    const long long N = (long long)(2 * l0 + 1) * dd + (long long)(2 * (l1 - l0)) * t, D = 2 * dd;
    return ramp_quotient(N, D, ramp_f32(N) * __builtin_amdgcn_rcpf((float)(unsigned long long)D));
}

// kRamp = false: rtdd_paint_strokes.  kRamp = true: rtdd_paint_ramp_strokes -- the same tiles, cull and walk; the record's fourth word
// carries label1 above label0 + 1, and a painting stroke whose two labels differ (and which is no stamp: both the same in every lane)
// evaluates ramp_label for the pixels it covers.  A compile-time variant: the constant-label kernel's code is what it was.
template <bool kRamp>
__global__ __launch_bounds__(256) void k_paint_strokes(const StrokeChunk C, uint8_t *__restrict__ edited, size_t editedPitch,
                                                       uint8_t *__restrict__ scribble, size_t scribblePitch,
                                                       const uint8_t *__restrict__ original, size_t originalPitch) {
    __shared__ int4 live[kStrokeChunk];           // the surviving strokes, unpacked: (the two ends, radius, brush | (label + 1) << 1 [| label1 << 10])
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int tx0 = C.x0 + (int)blockIdx.x * kPaintTileW, ty0 = C.y0 + (int)blockIdx.y * kPaintTileH;
    const int tx1 = min(tx0 + kPaintTileW - 1, C.x1), ty1 = min(ty0 + kPaintTileH - 1, C.y1);
    // cull: stroke `tid` against this tile
    bool keep = false;
    int4 rec = make_int4(0, 0, 0, 0);
    if (tid < C.count) {
        const PackedStroke q = C.s[tid];
        const int x0 = unpack_x(q.p0), y0 = unpack_y(q.p0), x1 = unpack_x(q.p1), y1 = unpack_y(q.p1);
        const int radius = (int)(q.meta & 0x7FF), h = radius / 2;
        keep = min(x0, x1) - h <= tx1 && max(x0, x1) + h >= tx0 && min(y0, y1) - h <= ty1 && max(y0, y1) + h >= ty0;
        rec = make_int4((int)q.p0, (int)q.p1, radius, (int)(q.meta >> 11));
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const int n = wave_count[w]; if (w < wave) base += n; total += n; }
    if (keep) live[base + __popcll(mask & ((1ull << lane) - 1))] = rec;
    __syncthreads();
    if (total == 0) return;
    const int x = tx0 + lane;
    if (x > tx1) return;
#pragma unroll
    for (int k = 0; k < kPaintTileH / 4; k++) {
        const int y = ty0 + wave + 4 * k;
        if (y > ty1) break;
        for (int i = total - 1; i >= 0; i--) {
            const int4 r = live[i];                                  // (one address for the whole wave: an LDS broadcast)
            if (!stroke_covers(x, y, r.x, r.y, r.z, r.w & 1)) continue;
            int label = (r.w >> 1) - 1;                              // RTDD_STROKE_ERASE = -1
            if constexpr (kRamp) {
                label = ((r.w >> 1) & 0x1FF) - 1;
                const int label1 = (r.w >> 10) & 0xFF;
                if (label >= 0 && label1 != label && r.x != r.y)     // (wave-uniform: the record is)
                    label = ramp_label(x, y, r.x, r.y, label, label1);
            }
            uint8_t *e = edited + (size_t)y * editedPitch + 3 * x;
            if (label >= 0) {
                e[0] = (uint8_t)label; e[1] = (uint8_t)label; e[2] = (uint8_t)label;
                scribble[(size_t)y * scribblePitch + x] = 255;
            } else {
                const uint8_t *o = original + (size_t)y * originalPitch + 3 * x;
                e[0] = o[0]; e[1] = o[1]; e[2] = o[2];
                scribble[(size_t)y * scribblePitch + x] = 0;
            }
            break;                                                   // the LAST stroke covering a pixel decides it
        }
    }
}

// rows of `width` bytes from one pitch to another (copy_h2d / copy_d2h, rtdd_live_submit: one side is a contiguous buffer whose row length is
// no multiple of four).  Four bytes per thread: one dword on whichever side allows it (gfx950 loads and stores dwords at any address:
// the dword goes to the side whose rows are NOT aligned only if that is the only way), bytes on the other; 8 MB in ~10 us.
typedef uint32_t __attribute__((aligned(1))) u32_any;
__global__ __launch_bounds__(256) void k_repitch(const uint8_t *__restrict__ src, size_t sp, uint8_t *__restrict__ dst, size_t dp, size_t width, int rows) {
    const size_t x = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int y0 = blockIdx.y * 8;
    if (x >= width) return;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (y0 + i >= rows) break;
        const uint8_t *s = src + (size_t)(y0 + i) * sp + x;
        uint8_t *d = dst + (size_t)(y0 + i) * dp + x;
        if (x + 3 < width) *(u32_any *)d = *(const u32_any *)s;
        else for (size_t k = 0; x + k < width; k++) d[k] = s[k];
    }
}

int launch_repitch(rtdd_ctx *ctx, hipStream_t stream, const void *src, size_t srcPitch, void *dst, size_t dstPitch, size_t widthBytes, int rows) {
    if (rows <= 0 || widthBytes == 0) return RTDD_OK;
    hipLaunchKernelGGL(k_repitch, dim3((unsigned)((widthBytes + 1023) / 1024), (unsigned)((rows + 7) / 8)), dim3(256), 0, stream, (const uint8_t *)src, srcPitch, (uint8_t *)dst, dstPitch, widthBytes, rows);
    RTDD_LAUNCH_CHECK(ctx, "k_repitch");
    return RTDD_OK;
}

static inline dim3 grid64x4(int rows, int cols, int images = 1) { return dim3((cols + 63) / 64, (rows + 3) / 4, images); }

int launch_convert(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, float *dst, size_t dstPitch,
                   const uint8_t *mask, size_t maskPitch, int rows, int cols, int images, size_t zSrc, size_t zDst, size_t zMask) {
    hipLaunchKernelGGL(k_convert, grid64x4(rows, cols, images), dim3(256), 0, ctx->stream, src, srcPitch, dst, dstPitch, mask, maskPitch, rows, cols, zSrc, zDst, zMask);
    RTDD_LAUNCH_CHECK(ctx, "k_convert");
    return RTDD_OK;
}

int launch_pyrdown_annotation(rtdd_ctx *ctx, const uint8_t *ps, size_t psp, const uint8_t *pe, size_t pep, int prows, int pcols,
                              uint8_t *cs, size_t csp, uint8_t *ce, size_t cep, int crows, int ccols, int images, size_t zPs, size_t zPe, size_t zCs, size_t zCe) {
    hipLaunchKernelGGL(k_pyrdown_annotation, grid64x4(crows, ccols, images), dim3(256), 0, ctx->stream, ps, psp, pe, pep, prows, pcols, cs, csp, ce, cep, crows, ccols, zPs, zPe, zCs, zCe);
    RTDD_LAUNCH_CHECK(ctx, "k_pyrdown_annotation");
    return RTDD_OK;
}

// the kernel for a pyramid of top + 1 levels: the chain in LDS where it is asked for (RTDD_OPT_ANNOTATION_LDS) and compiled (two to six
// levels), through global memory otherwise
using AnnotationKernel = void (*)(AnnotationPyramid);
template <bool kRebuild>
static AnnotationKernel annotation_kernel(bool lds, int top) {
    static constexpr AnnotationKernel in_lds[] = {k_annotation_pyramid_lds<1, kRebuild>, k_annotation_pyramid_lds<2, kRebuild>, k_annotation_pyramid_lds<3, kRebuild>,
                                                  k_annotation_pyramid_lds<4, kRebuild>, k_annotation_pyramid_lds<5, kRebuild>};
    return lds && top >= 1 && top <= 5 ? in_lds[top - 1] : k_annotation_pyramid<kRebuild>;
}

int launch_annotation_pyramid(rtdd_ctx *ctx, int levels, uint8_t *const *scribble, const size_t *sp, const size_t *zs, uint8_t *const *edited, const size_t *ep, const size_t *ze,
                              const int *rows, const int *cols, float *depth, size_t dp, size_t zd, int images, bool rebuild) {
    if (levels < 1 || levels > kApMaxLevels) return fail(ctx, RTDD_ERR_INVALID, "annotation pyramid: too many levels");
    AnnotationPyramid A{};
    A.levels = levels;
    for (int l = 0; l < levels; l++) { A.scribble[l] = scribble[l]; A.edited[l] = edited[l]; A.sp[l] = sp[l]; A.ep[l] = ep[l]; A.zs[l] = zs[l]; A.ze[l] = ze[l]; A.rows[l] = rows[l]; A.cols[l] = cols[l]; }
    A.depth = depth; A.dp = dp; A.zd = zd;
    // tiles of kApB x kApB coarsest pixels, one tile more than the coarsest level needs in either direction: the finer levels' last
    // pixels (their sizes are floors) lie under coarsest pixels that do not exist
    const int top = levels - 1;
    int gx = 1, gy = 1;
    for (int l = 1; l <= top; l++) {                                 // the largest tile index any level's last pixel falls into
        const int f = 1 << (top - l);
        const int tx = (cols[l] - 1 + f - 1) / f / kApB + 1, ty = (rows[l] - 1 + f - 1) / f / kApB + 1;
        if (cols[l] > 0 && tx > gx) gx = tx;
        if (rows[l] > 0 && ty > gy) gy = ty;
    }
    if (top == 0) { gx = (cols[0] + kApB - 1) / kApB; gy = (rows[0] + kApB - 1) / kApB; }
    if (gx < 1 || gy < 1) return RTDD_OK;
    const dim3 grid(gx, gy, images);
    if (rebuild) {
        hipLaunchKernelGGL(annotation_kernel<true>(ctx->opt.annotation_lds, top), grid, dim3(256), 0, ctx->stream, A);
        RTDD_LAUNCH_CHECK(ctx, "k_annotation_rebuild");
    } else {
        hipLaunchKernelGGL(annotation_kernel<false>(ctx->opt.annotation_lds, top), grid, dim3(256), 0, ctx->stream, A);
        RTDD_LAUNCH_CHECK(ctx, "k_annotation_pyramid");
    }
    return RTDD_OK;
}

int launch_paint(rtdd_ctx *ctx, int x, int y, int color, int radius, const PaintTarget &t) {
    const int h = radius / 2;                          // C integer division, as the reference (:58-59)
    const int x0 = x - h < 0 ? 0 : x - h, y0 = y - h < 0 ? 0 : y - h;
    const int x1 = x + h > t.cols - 1 ? t.cols - 1 : x + h, y1 = y + h > t.rows - 1 ? t.rows - 1 : y + h;
    if (x1 < x0 || y1 < y0) return RTDD_OK;            // brush entirely outside the image (or negative radius)
    hipLaunchKernelGGL(k_paint, grid64x4(y1 - y0 + 1, x1 - x0 + 1), dim3(256), 0, ctx->stream, x0, y0, x1, y1, color, t.edited, t.editedPitch, t.scribble, t.scribblePitch);
    RTDD_LAUNCH_CHECK(ctx, "k_paint");
    return RTDD_OK;
}

// strokes: checked by rtdd_paint_strokes / rtdd_paint_ramp_strokes (image_api.cpp) -- coordinates, radius, brush and labels inside the packed
// fields' ranges.  One body for both record types: the labels' bits and the kernel's variant are all that differs.
static uint32_t pack_labels(const rtdd_stroke &q) { return (uint32_t)(q.label + 1) << 12; }
static uint32_t pack_labels(const rtdd_ramp_stroke &q) { return (uint32_t)(q.label0 + 1) << 12 | (uint32_t)std::max(q.label1, 0) << 21; }

template <class Stroke>
int launch_paint_strokes(rtdd_ctx *ctx, const Stroke *strokes, int count, const PaintTarget &t) {
    constexpr bool ramp = std::is_same<Stroke, rtdd_ramp_stroke>::value;
    for (int first = 0; first < count; first += kStrokeChunk) {
        StrokeChunk C;
        C.count = count - first < kStrokeChunk ? count - first : kStrokeChunk;
        C.x0 = t.cols; C.y0 = t.rows; C.x1 = -1; C.y1 = -1;          // union of the strokes' boxes, each clipped to the image
        for (int i = 0; i < C.count; i++) {
            const Stroke &q = strokes[first + i];
            const int h = q.radius / 2;
            const int x0 = std::max(std::min(q.x0, q.x1) - h, 0), x1 = std::min(std::max(q.x0, q.x1) + h, t.cols - 1);
            const int y0 = std::max(std::min(q.y0, q.y1) - h, 0), y1 = std::min(std::max(q.y0, q.y1) + h, t.rows - 1);
            if (x0 <= x1 && y0 <= y1) { C.x0 = std::min(C.x0, x0); C.x1 = std::max(C.x1, x1); C.y0 = std::min(C.y0, y0); C.y1 = std::max(C.y1, y1); }
            C.s[i] = PackedStroke{pack_xy(q.x0, q.y0), pack_xy(q.x1, q.y1), (uint32_t)q.radius | ((uint32_t)q.brush << 11) | pack_labels(q)};
        }
        for (int i = C.count; i < kStrokeChunk; i++) C.s[i] = PackedStroke{0, 0, 0};
        dim3 grid;
        if (!paint_grid(C.x0, C.y0, C.x1, C.y1, t.rows, t.cols, grid)) continue;        // every stroke of the chunk lies outside the image
        hipLaunchKernelGGL(k_paint_strokes<ramp>, grid, dim3(256), 0, ctx->stream, C, t.edited, t.editedPitch, t.scribble, t.scribblePitch, t.original, t.originalPitch);
        RTDD_LAUNCH_CHECK(ctx, "k_paint_strokes");
    }
    return RTDD_OK;
}
template int launch_paint_strokes(rtdd_ctx *, const rtdd_stroke *, int, const PaintTarget &);
template int launch_paint_strokes(rtdd_ctx *, const rtdd_ramp_stroke *, int, const PaintTarget &);

}  // namespace rtdd
