// rtdd_fill_similar (extension, include/rtdd.h): the magic wand -- every pixel joined to the clicked one through pixels whose colour is
// within `tolerance` of the clicked colour gets the fill's label, ramp or erasure.  The covered set is a connected component: the unique
// fixpoint of "an eligible pixel beside a reached pixel is reached", so every correct schedule writes the same bytes.
//
// Two bit planes in the context's table buffer (ctx->sat), one 64-bit word per 64 pixels of a row, W = ceil(cols / 64) words per row:
//   eligible   bit x & 63 of word (y, x >> 6): max(|B - sB|, |G - sG|, |R - sR|) <= tolerance against the seed's colour; bits at or
//              beyond `cols` in a row's last word are 0, so nothing is ever reached there
//   reach      the seed's bit, grown to the fixpoint (RTDD_WAND_GLOBAL: the eligible plane itself, nothing to grow)
//   k_wand_mask   both planes: a wave's __ballot of the comparison per word; also the result words
//   k_wand_grow   one pass over the whole image per launch; a wave owns 64 columns x 64 rows, lane = row, and runs ITS block to the
//                 block's own fixpoint in registers against a halo read once.  The host queues kWandRound passes, reads their counters
//                 back and stops at the first pass that changed nothing.
//   k_wand_paint  the paint calls' 64 x 16 tile over the image: fill_polygon.hip's write under the reach bit, the pixel count and the
//                 bounding box reduced per tile in LDS, then by vector atomics
// Why racing reads are safe.  Only its owner stores a reach word; a neighbour's wave reads it for its halo, in the same launch, with no
// ordering.  Reach only ever grows and every bit set is a true member of the component, so whatever mixture of old and new the read
// returns is a SUBSET of the truth: it can delay a bit by a pass, never set a wrong one.  A pass in which no wave changed a word proves
// the fixpoint: nobody wrote, so every halo read in it was of the final state, and every block was at its own fixpoint against it.
//
// rtdd_fill_surface (extension, include/rtdd.h): the same wand on the depth map -- two neighbours are joined when their clamped depths
// differ by at most `step` and both lie in the band around the clicked depth.  A link is a property of a PAIR of pixels, so no
// eligibility plane can state it: three planes, laid out as above,
//   H          bit x: the link (x, y) - (x + 1, y); 0 for the last column and at or beyond `cols`
//   V          bit x: the link (x, y) - (x, y + 1); 0 for the last row and at or beyond `cols`
//   reach      the seed's bit, grown to the fixpoint (RTDD_SURFACE_GLOBAL: the admissible plane itself; H and V are not built)
//   k_surface_links   the planes: a wave owns one word's columns over kSurfaceStrip rows and keeps the row below in registers for the
//                     next round, so a row is loaded once (and once more per strip); the right neighbour comes by a lane shift
//   k_surface_grow    k_wand_grow's pass with the link fill in place of the eligibility fill: the same block, halo, loop and counter,
//                     and the same argument for the racing reads (reach only grows, every bit set is true; H and V are constant)
//   k_wand_paint      itself, with the same result words and host fold; the host's loop over rounds of passes is the wand's
//                     (wand_grow_rounds)
// 4-connectivity only: a diagonal link would be two more planes (one per diagonal) and two more loads per row of the grow pass.
#include <climits>
#include <cmath>

#include "effect_common.hpp"
#include "paint_common.hpp"

namespace rtdd {

constexpr int kWandRound = 8;             // grow passes queued between two read-backs of their counters (profiles/r20_wand.txt)
constexpr int kWandBlock = 64;            // rows (= lanes) and columns (= bits) of a wave's block
// The result words: kWandSlots records of box and count, each on a cache line of its own; a tile of k_wand_paint adds its own to record
// number-of-tile mod kWandSlots and the host folds them.  Thousands of atomics on ONE address serialise: 5 per wave on 5 words cost
// 440 us at 1080p for a selection of 2 M pixels, 50 times the launch; once per tile, and the bounds only where they beat a plain load,
// still 100 us (every tile of a launch runs at once and sees the initial value) (EXPERIMENTS.md, profiles/r20_wand.txt).
constexpr int kWandSlots = 64, kWandSlotStride = 32;
enum { kWandX0 = 0, kWandY0, kWandX1, kWandY1, kWandPixels, kWandInfoWords = kWandSlots * kWandSlotStride };
__host__ __device__ inline int wand_info_init(int k) { return k == kWandX0 || k == kWandY0 ? INT_MAX : k == kWandPixels ? 0 : -1; }

struct WandArgs {
    int rows, cols, W;                      // W: words per row of a bit plane
    int label0;                             // 0..255, or RTDD_STROKE_ERASE
    int ramp;                               // as FillArgs (fill_polygon.hip): label0 != label1 on an axis with length
    int ax0, ay0, adx, ady;
    long long dd, A;                        // adx^2 + ady^2;  (2 label0 + 1) dd
    int B;                                  // 2 (label1 - label0)
};

// k_fill_polygon's label (fill_polygon.hip: fill_label, with the same bounds -- the axis and the pixel lie in the same domain)
__device__ __forceinline__ int wand_label(int px, int py, const WandArgs &C, float rcpD) {
    const long long vx = px - C.ax0, vy = py - C.ay0;
    const long long t = min(max(vx * C.adx + vy * C.ady, 0ll), C.dd);
    const long long N = C.A + (long long)C.B * t;
    return ramp_quotient(N, 2 * C.dd, ramp_f32(N) * rcpD);
}

// One wave per word: rows y = 4 blockIdx.y + wave, columns 64 blockIdx.x + lane.  The seed lies inside the image (checked by the caller).
__global__ __launch_bounds__(256) void k_wand_mask(const uint8_t *__restrict__ original, size_t op, int rows, int cols, int W, int sx, int sy,
                                                   int tolerance, int global, u64 *__restrict__ elig, u64 *__restrict__ reach, int *__restrict__ info) {
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < kWandInfoWords; i += 256) info[i] = wand_info_init(i % kWandSlotStride);
    const int y = (int)blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform: the ballot below has its whole wave
    const int lane = threadIdx.x & 63, x = (int)blockIdx.x * 64 + lane;
    const uint8_t *s = original + (size_t)sy * op + 3 * (size_t)sx;  // (the same address in every lane)
    const int sB = s[0], sG = s[1], sR = s[2];
    bool ok = false;
    if (x < cols) {
        const uint8_t *p = original + (size_t)y * op + 3 * (size_t)x;
        ok = max(max(abs((int)p[0] - sB), abs((int)p[1] - sG)), abs((int)p[2] - sR)) <= tolerance;
    }
    const u64 e = __ballot(ok);
    if (lane == 0) {
        const size_t i = (size_t)y * W + blockIdx.x;
        elig[i] = e;
        reach[i] = global ? e : (y == sy && (int)blockIdx.x == (sx >> 6) ? 1ull << (sx & 63) : 0ull);
    }
}

// every eligible bit joined to a bit of r (r a subset of e) through eligible bits, towards higher bits: adding r to e carries through
// each run of ones from its lowest reached bit; the bits the sum changed inside e are the run above it
__device__ __forceinline__ u64 wand_fill_up(u64 e, u64 r) { return r | (((e + r) ^ e) & e); }
__device__ __forceinline__ u64 wand_fill_row(u64 e, u64 r) {
    r = wand_fill_up(e, r);
    return __brevll(wand_fill_up(__brevll(e), __brevll(r)));
}

// One pass.  Workgroup: four waves, four neighbouring blocks of one block row; they share nothing.  `prev`: the counter of the pass
// before (final by stream order; null for the first pass of a call): 0 says the fixpoint was reached, every wave leaves at once.
// The loop's lane exchanges need the whole wave: no lane leaves before the loop ends, and the exit is a ballot's, wave-uniform.  It is
// bounded: an iteration that does not end the loop sets at least one of the block's 4096 bits.
__global__ __launch_bounds__(256) void k_wand_grow(const u64 *__restrict__ elig, u64 *reach, int rows, int W, int connect8, const int *prev, int *mine) {
    if (prev && *prev == 0) return;
    const int bx = (int)blockIdx.x * 4 + wave_id();
    if (bx >= W) return;                                             // wave-uniform
    const int lane = threadIdx.x & 63, y0 = (int)blockIdx.y * kWandBlock, y = y0 + lane;
    const bool in = y < rows;
    auto word = [&](int yy, int xx) -> u64 { return yy >= 0 && yy < rows && xx >= 0 && xx < W ? reach[(size_t)yy * W + xx] : 0ull; };
    const u64 e = in ? elig[(size_t)y * W + bx] : 0ull;
    const u64 r0 = word(y, bx);
    // the halo, read once: bit 63 of the word to the left and bit 0 of the word to the right of this row (as bits 0 and 63: where they
    // touch), and the row above the block (in lane 0) and below it (in lane 63) with their own two side bits
    const u64 side = (word(y, bx - 1) >> 63) | (word(y, bx + 1) << 63);
    const int hy = lane == 0 ? y0 - 1 : y0 + kWandBlock;             // (used by lanes 0 and 63 only)
    const bool edge = lane == 0 || lane == 63;
    const u64 hrow = edge ? word(hy, bx) : 0ull;
    const u64 hside = edge && connect8 ? (word(hy, bx - 1) >> 63) | (word(hy, bx + 1) << 63) : 0ull;
    if (__ballot((r0 | side | hrow | hside) != 0) == 0) return;      // nothing reached in the block or around it
    // the side bits of the rows above and below each lane's: fixed for the launch
    u64 side_ud = 0;
    if (connect8) {
        const u64 up = __shfl_up(side, 1), dn = __shfl_down(side, 1);
        side_ud = (lane == 0 ? hside : up) | (lane == 63 ? hside : dn);
    }
    u64 r = r0;
    for (;;) {
        const u64 up = __shfl_up(r, 1), dn = __shfl_down(r, 1);
        u64 v = (lane == 0 ? hrow : up) | (lane == 63 ? hrow : dn);  // reached in the rows above and below
        if (connect8) v |= (v << 1) | (v >> 1) | side_ud;            // ... and diagonally
        const u64 next = wand_fill_row(e, r | (e & (v | side)));
        const bool grew = next != r;
        r = next;
        if (__ballot(grew) == 0) break;
    }
    const bool changed = r != r0;
    if (changed) reach[(size_t)y * W + bx] = r;                      // (r != 0 only where e != 0: inside the image)
    if (__ballot(changed) != 0 && lane == 0) atomicAdd(mine, 1);
}

// ---- rtdd_fill_surface ----
constexpr int kSurfaceStrip = 8;          // consecutive rows of one word's columns that a wave of k_surface_links walks

// One wave per word and strip: rows (4 blockIdx.y + wave) kSurfaceStrip ..., columns 64 blockIdx.x + lane.  The seed lies inside the image
// and depthPitch is a multiple of 4 (checked by the caller).  `cur` is d' of the lane's pixel; the row below, loaded for the V links,
// is the next round's `cur`.  Nothing is read outside the image: the right neighbour only where x + 1 < cols, the row below only where
// y + 1 < rows.
__global__ __launch_bounds__(256) void k_surface_links(const float *__restrict__ depth, size_t depthPitch, int rows, int cols, int W, int sx, int sy,
                                                       float step, float below, float above, int global, u64 *__restrict__ H, u64 *__restrict__ V,
                                                       u64 *__restrict__ reach, int *__restrict__ info) {
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < kWandInfoWords; i += 256) info[i] = wand_info_init(i % kWandSlotStride);
    const int y0 = ((int)blockIdx.y * 4 + wave_id()) * kSurfaceStrip;
    if (y0 >= rows) return;                                          // wave-uniform: the ballots below have their whole wave
    const int lane = threadIdx.x & 63, x = (int)blockIdx.x * 64 + lane;
    auto at = [&](int yy, int xx) { return remove_depth(((const float *)((const char *)depth + (size_t)yy * depthPitch))[xx]); };
    const float ds = at(sy, sx);                                     // (the same address in every lane)
    const float lo = ds - below, hi = ds + above;
    const bool inx = x < cols, right_in = x + 1 < cols;
    float cur = inx ? at(y0, x) : 0.0f;
    for (int k = 0; k < kSurfaceStrip; k++) {
        const int y = y0 + k;
        if (y >= rows) break;                                        // wave-uniform
        const bool down_in = y + 1 < rows;
        float right = __shfl_down(cur, 1);
        if (lane == 63) right = right_in ? at(y, x + 1) : 0.0f;
        const float down = inx && down_in ? at(y + 1, x) : 0.0f;
        const bool a = inx && lo <= cur && cur <= hi;
        const size_t i = (size_t)y * W + blockIdx.x;
        if (global) {
            const u64 aw = __ballot(a);
            if (lane == 0) reach[i] = aw;
        } else {
            const u64 hw = __ballot(a && right_in && lo <= right && right <= hi && fabsf(cur - right) <= step);
            const u64 vw = __ballot(a && down_in && lo <= down && down <= hi && fabsf(cur - down) <= step);
            if (lane == 0) {
                H[i] = hw; V[i] = vw;
                reach[i] = y == sy && (int)blockIdx.x == (sx >> 6) ? 1ull << (sx & 63) : 0ull;
            }
        }
        cur = down;
    }
}

// every bit joined to a bit of r through link bits, towards higher bits: bit x of h links x to x + 1, so adding the reached link bits to
// h carries through each run of links from its lowest reached one and lands on the pixel above the run -- which is reached; the carry
// out of bit 63 (the link into the next word) is dropped: that word's wave picks it up through its side bit.  Towards lower bits the
// same on the reversed words, the link x - (x + 1) then lying at the reversed index of x + 1: one further down.
__device__ __forceinline__ u64 surface_fill_up(u64 h, u64 r) { return r | ((h + (r & h)) ^ h); }
__device__ __forceinline__ u64 surface_fill_row(u64 h, u64 r) {
    r = surface_fill_up(h, r);
    return __brevll(surface_fill_up(__brevll(h) >> 1, __brevll(r)));
}

// One pass: k_wand_grow's, under 4-connectivity, with links.  A reached neighbour counts where the link to it is set: the word to the
// left under bit 63 of ITS H word, the word to the right under bit 63 of the own one, the row above under its V word, the row below
// under the own one.
__global__ __launch_bounds__(256) void k_surface_grow(const u64 *__restrict__ H, const u64 *__restrict__ V, u64 *reach, int rows, int W, const int *prev, int *mine) {
    if (prev && *prev == 0) return;
    const int bx = (int)blockIdx.x * 4 + wave_id();
    if (bx >= W) return;                                             // wave-uniform
    const int lane = threadIdx.x & 63, y0 = (int)blockIdx.y * kWandBlock, y = y0 + lane;
    const bool in = y < rows;
    auto word = [&](const u64 *plane, int yy, int xx) -> u64 { return yy >= 0 && yy < rows && xx >= 0 && xx < W ? plane[(size_t)yy * W + xx] : 0ull; };
    const u64 h = word(H, y, bx), v = word(V, y, bx);
    const u64 r0 = word(reach, y, bx);
    // the halo, read once, each bit under its link: the two side bits of this row (as bits 0 and 63: where they touch), and the row
    // above the block (in lane 0) and below it (in lane 63)
    const u64 side = ((word(reach, y, bx - 1) & word(H, y, bx - 1)) >> 63) | ((word(reach, y, bx + 1) << 63) & h);
    const u64 habove = lane == 0 ? word(reach, y0 - 1, bx) & word(V, y0 - 1, bx) : 0ull;
    const u64 hbelow = lane == 63 ? word(reach, y0 + kWandBlock, bx) & v : 0ull;
    if (__ballot((r0 | side | habove | hbelow) != 0) == 0) return;   // nothing reached in the block or around it
    u64 r = r0;
    for (;;) {
        const u64 up = __shfl_up(r & v, 1), dn = __shfl_down(r, 1) & v;
        const u64 next = surface_fill_row(h, r | side | (lane == 0 ? habove : up) | (lane == 63 ? hbelow : dn));
        const bool grew = next != r;
        r = next;
        if (__ballot(grew) == 0) break;
    }
    const bool changed = r != r0;
    if (changed && in) reach[(size_t)y * W + bx] = r;                // (r != 0 only where a link ends: inside the image)
    if (__ballot(changed) != 0 && lane == 0) atomicAdd(mine, 1);
}

// k_fill_polygon's tile and write (fill_polygon.hip) under the reach bit; x0 = y0 = 0: the launch covers the image
__global__ __launch_bounds__(256) void k_wand_paint(const WandArgs C, const u64 *__restrict__ reach, uint8_t *__restrict__ edited, size_t editedPitch,
                                                    uint8_t *__restrict__ scribble, size_t scribblePitch,
                                                    const uint8_t *__restrict__ original, size_t originalPitch, int *__restrict__ info) {
    __shared__ int tile[5];                                          // the tile's box and count (no thread leaves before the end: barriers)
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int x = (int)blockIdx.x * kPaintTileW + lane, ty0 = (int)blockIdx.y * kPaintTileH;
    if (threadIdx.x < 5) tile[threadIdx.x] = wand_info_init(threadIdx.x);
    __syncthreads();
    const float rcpD = C.ramp ? __builtin_amdgcn_rcpf((float)(unsigned long long)(2 * C.dd)) : 0.0f;
    int pixels = 0, ya = INT_MAX, yb = -1;
    u64 any = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int y = ty0 + wave + 4 * k;
        if (y >= C.rows) break;
        const u64 w = reach[(size_t)y * C.W + blockIdx.x];             // (one address for the wave)
        if (w == 0) continue;
        pixels += __popcll(w); any |= w; ya = min(ya, y); yb = y;
        if (!((w >> lane) & 1)) continue;                            // (a reach bit lies below `cols`)
        uint8_t *e = edited + (size_t)y * editedPitch + 3 * x;
        if (C.label0 >= 0) {
            const int label = C.ramp ? wand_label(x, y, C, rcpD) : C.label0;
            e[0] = (uint8_t)label; e[1] = (uint8_t)label; e[2] = (uint8_t)label;
            scribble[(size_t)y * scribblePitch + x] = 255;
        } else {
            const uint8_t *o = original + (size_t)y * originalPitch + 3 * x;
            e[0] = o[0]; e[1] = o[1]; e[2] = o[2];
            scribble[(size_t)y * scribblePitch + x] = 0;
        }
    }
    if (lane == 0 && any) {                                          // the wave's rows, in LDS
        const int xb = (int)blockIdx.x * kPaintTileW;
        atomicAdd(&tile[kWandPixels], pixels);
        atomicMin(&tile[kWandX0], xb + __ffsll((unsigned long long)any) - 1); atomicMax(&tile[kWandX1], xb + 63 - __clzll((long long)any));
        atomicMin(&tile[kWandY0], ya); atomicMax(&tile[kWandY1], yb);
    }
    __syncthreads();
    if (threadIdx.x == 0 && tile[kWandPixels] > 0) {                 // the tile's, into its record
        int *slot = info + (blockIdx.y * gridDim.x + blockIdx.x) % kWandSlots * kWandSlotStride;
        atomicAdd(&slot[kWandPixels], tile[kWandPixels]);
        atomicMin(&slot[kWandX0], tile[kWandX0]); atomicMin(&slot[kWandY0], tile[kWandY0]);
        atomicMax(&slot[kWandX1], tile[kWandX1]); atomicMax(&slot[kWandY1], tile[kWandY1]);
    }
}

// ---- host: what the two wands share ----
// the u32 words of the table buffer behind `planes` bit planes: the result records and a round's counters
static size_t wand_words(size_t plane, int planes) { return 2 * planes * plane + kWandInfoWords + kWandRound; }

// Rounds of kWandRound passes, each pass launched (and its launch checked) by launch(prev, mine) with the counter of the pass before (null for the first of the
// call) and its own, until a pass changed nothing; the counters are read back once per round.  SYNCHRONISES.
template <class Launch>
static int wand_grow_rounds(rtdd_ctx *ctx, const PaintTarget &t, int *counters, long long &passes, Launch launch) {
    const long long limit = (long long)t.rows * t.cols + 1;          // every pass short of the fixpoint adds a pixel
    for (bool done = false; !done;) {
        if (passes >= limit) return fail(ctx, RTDD_ERR_STATE, "wand: no fixpoint within rows * cols + 1 passes (cannot happen: every pass short of it adds a pixel)");
        RTDD_HIP(ctx, hipMemsetAsync(counters, 0, kWandRound * sizeof(int), ctx->stream));
        for (int p = 0; p < kWandRound; p++) {
            RTDD_TRY(launch(p > 0 ? counters + p - 1 : nullptr, counters + p));
        }
        int host[kWandRound];
        RTDD_HIP(ctx, hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
        RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int p = 0; p < kWandRound && !done; p++) { passes++; done = host[p] == 0; }
    }
    return RTDD_OK;
}

// k_wand_paint under the grown plane, the result records folded on the host.  SYNCHRONISES.
static int wand_paint(rtdd_ctx *ctx, const PaintTarget &t, int W, int ax0, int ay0, int ax1, int ay1, int label0, int label1, const u64 *reach,
                      int *info, long long passes, rtdd_wand_info *out) {
    WandArgs C{};
    C.rows = t.rows; C.cols = t.cols; C.W = W;
    C.label0 = label0;
    C.ax0 = ax0; C.ay0 = ay0; C.adx = ax1 - ax0; C.ady = ay1 - ay0;
    C.dd = (long long)C.adx * C.adx + (long long)C.ady * C.ady;
    C.ramp = label0 >= 0 && label0 != label1 && C.dd != 0;
    C.A = (long long)(2 * label0 + 1) * C.dd;
    C.B = 2 * (label1 - label0);
    hipLaunchKernelGGL(k_wand_paint, dim3(W, (t.rows + kPaintTileH - 1) / kPaintTileH), dim3(256), 0, ctx->stream, C, reach, t.edited, t.editedPitch,
                       t.scribble, t.scribblePitch, t.original, t.originalPitch, info);
    RTDD_LAUNCH_CHECK(ctx, "k_wand_paint");
    int host[kWandInfoWords];
    RTDD_HIP(ctx, hipMemcpyAsync(host, info, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int r[5];
    for (int k = 0; k < 5; k++) r[k] = wand_info_init(k);
    for (int i = 0; i < kWandSlots; i++) {
        const int *slot = host + i * kWandSlotStride;
        r[kWandPixels] += slot[kWandPixels];
        r[kWandX0] = std::min(r[kWandX0], slot[kWandX0]); r[kWandY0] = std::min(r[kWandY0], slot[kWandY0]);
        r[kWandX1] = std::max(r[kWandX1], slot[kWandX1]); r[kWandY1] = std::max(r[kWandY1], slot[kWandY1]);
    }
    if (out) *out = rtdd_wand_info{r[kWandPixels], r[kWandX0], r[kWandY0], r[kWandX1], r[kWandY1], (int)std::min<long long>(passes, INT_MAX)};
    return RTDD_OK;
}

// checked by rtdd_fill_similar (image_api.cpp): the seed inside the image, tolerance, flags, labels and axis valid, all three images given.
// Synchronises: the number of grow passes depends on the data.
int launch_fill_similar(rtdd_ctx *ctx, const rtdd_wand &wand, const PaintTarget &t, rtdd_wand_info *out) {
    const int W = (t.cols + 63) / 64;
    const size_t plane = (size_t)t.rows * W;                         // (at most 2^15 * 2^9 words)
    if (ensure_sat(ctx, wand_words(plane, 2)) != RTDD_OK) {
        (void)hipGetLastError();
        return fail(ctx, RTDD_ERR_NOMEM, "fill_similar: the two bit planes could not be allocated");
    }
    ctx->sat_rows = ctx->sat_cols = 0;                               // whatever table lay here is gone: the next table-path defocus zeroes its padding again
    u64 *elig = (u64 *)ctx->sat, *reach = elig + plane;
    int *info = (int *)(reach + plane), *counters = info + kWandInfoWords;
    const int global = (wand.flags & RTDD_WAND_GLOBAL) != 0, connect8 = (wand.flags & RTDD_WAND_CONNECT_8) != 0;
    hipLaunchKernelGGL(k_wand_mask, dim3(W, (t.rows + 3) / 4), dim3(256), 0, ctx->stream, t.original, t.originalPitch, t.rows, t.cols, W, wand.x, wand.y,
                       wand.tolerance, global, elig, reach, info);
    RTDD_LAUNCH_CHECK(ctx, "k_wand_mask");
    long long passes = 0;
    if (!global) {
        const dim3 grid((W + 3) / 4, (t.rows + kWandBlock - 1) / kWandBlock);
        RTDD_TRY(wand_grow_rounds(ctx, t, counters, passes, [&](const int *prev, int *mine) {
            hipLaunchKernelGGL(k_wand_grow, grid, dim3(256), 0, ctx->stream, elig, reach, t.rows, W, connect8, prev, mine);
            RTDD_LAUNCH_CHECK(ctx, "k_wand_grow");
            return (int)RTDD_OK;
        }));
    }
    return wand_paint(ctx, t, W, wand.ax0, wand.ay0, wand.ax1, wand.ay1, wand.label0, wand.label1, reach, info, passes, out);
}

// checked by rtdd_fill_surface (image_api.cpp): the seed inside the image; step, band, flags, labels and axis valid; the depth map given
// and aligned.  Synchronises, as launch_fill_similar.
int launch_fill_surface(rtdd_ctx *ctx, const rtdd_surface_wand &wand, const PaintTarget &t, const float *depth, size_t depthPitch, rtdd_wand_info *out) {
    const int W = (t.cols + 63) / 64;
    const size_t plane = (size_t)t.rows * W;
    if (ensure_sat(ctx, wand_words(plane, 3)) != RTDD_OK) {
        (void)hipGetLastError();
        return fail(ctx, RTDD_ERR_NOMEM, "fill_surface: the three bit planes could not be allocated");
    }
    ctx->sat_rows = ctx->sat_cols = 0;                               // (as launch_fill_similar)
    u64 *H = (u64 *)ctx->sat, *V = H + plane, *reach = V + plane;
    int *info = (int *)(reach + plane), *counters = info + kWandInfoWords;
    const int global = (wand.flags & RTDD_SURFACE_GLOBAL) != 0;
    hipLaunchKernelGGL(k_surface_links, dim3(W, (t.rows + 4 * kSurfaceStrip - 1) / (4 * kSurfaceStrip)), dim3(256), 0, ctx->stream, depth, depthPitch,
                       t.rows, t.cols, W, wand.x, wand.y, wand.step, wand.below, wand.above, global, H, V, reach, info);
    RTDD_LAUNCH_CHECK(ctx, "k_surface_links");
    long long passes = 0;
    if (!global) {
        const dim3 grid((W + 3) / 4, (t.rows + kWandBlock - 1) / kWandBlock);
        RTDD_TRY(wand_grow_rounds(ctx, t, counters, passes, [&](const int *prev, int *mine) {
            hipLaunchKernelGGL(k_surface_grow, grid, dim3(256), 0, ctx->stream, H, V, reach, t.rows, W, prev, mine);
            RTDD_LAUNCH_CHECK(ctx, "k_surface_grow");
            return (int)RTDD_OK;
        }));
    }
    return wand_paint(ctx, t, W, wand.ax0, wand.ay0, wand.ax1, wand.ay1, wand.label0, wand.label1, reach, info, passes, out);
}

}  // namespace rtdd
