// bokeh.hip -- the occlusion-aware lens blur (rtdd_simulate_bokeh, include/rtdd.h; DESIGN.md section 4 "Bokeh"): every SOURCE pixel
// spreads its colour over its own circle of confusion, and a source behind the target spreads no wider than the target's own circle --
// evaluated as a gather.  No reference behaviour: the definition is the header's, restated twice in tests/bokeh_ref.py.  One launch.
//
// A bounded gather from LDS, k_ambient_occlusion's shape.  A workgroup owns a tile of 64 x 16 pixels and stages ONE packed word per
// pixel of the tile and of a halo of h = K / 2 pixels on every side: B | G << 8 | R << 16 | (s & 255) << 24, s the signed circle of
// confusion (|s| <= K <= 127), clamped, subtracted, scaled and divided once per pixel, not once per sample.  A position outside the
// image is staged as s = -128, a value no pixel has: it is never "behind" a target (s_q > s_p is false), so its ke is its own 128, and
// wt[128] == 0 -- a source that adds nothing to any sum; the inner loop holds no bounds test.  One barrier orders the staging before
// the gather; nothing returns in front of it.  Then a wave takes a row of the tile, its lanes 64 consecutive x: at every window offset
// the wave reads 64 consecutive LDS words, free of bank conflicts whatever the pitch.
//
// The window is bounded by the largest |s| the workgroup staged (a source further than that / 2 reaches nothing, and no target's cap
// admits more): every wave reduces its own, one word per wave crosses the barrier, and the loop walks the disc of that diameter, row
// by row.  A tile that staged no |s| > 1 copies the original from its own words.
//
// The tile is the same for every K, the LDS array and the workgroup are not: the array holds the halo of the largest h of its class --
// 8, 16, 32 or 63: 10, 18, 40 and 106 KiB of the CU's 160 -- and the workgroup is 4, 4, 8 or 16 waves as k_ambient_occlusion's.  Within
// a class only the halo K needs is staged.  The weights wt[k] = floor(2^30 / N(k)) are a constant table of the code object, computed by
// the compiler, copied to LDS beside the tile.
//
// All arithmetic behind s is integer: W and the three S_c are 64-bit sums of 32 x 32-bit products (S_c < 2^52), exact in any order, so
// the bytes do not depend on RTDD_OPT_FP_CONTRACT or on the order of the walk.  The one 64-bit division per channel and pixel is
// outside the loop.
//
// Resources (hipcc's report for gfx950, every instantiation): 35 - 41 VGPRs, no scratch, no spills; 10.5, 18.5, 40.5 and 106 KiB of LDS.
// The inner loop, unrolled by four, in the disassembly: 17 VALU instructions per sample -- 8 for ke and the reach test out of the
// source word's top byte (SDWA), 1 for the weight's address, 3 for the colour bytes, 3 v_mad_u64_u32 (quarter rate) and the 64-bit add
// of W, 1 of addressing -- and two ds_read_b32, the source word and its weight; the four source words of a step are read together.
// Measured (profiles/r16_bokeh.txt): 1.2 - 1.8 T samples/s, 0.37 ms at 1080p with the default aperture.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

constexpr int kBkW = 64, kBkH = 16;                                 // the tile: a wave's 64 lanes wide
constexpr int kBkMaxK = 127;                                        // s fits 8 bits; the tile with its halo fits LDS
constexpr int kBkCodes = kBkMaxK + 2;                               // wt[0 .. 127] and the outside code's wt[128] == 0
constexpr uint32_t kBkOutside = 0x80000000u;                        // s == -128, no colour

// N(k): the integer (dx, dy) with 4 (dx^2 + dy^2) <= k^2, that is dx^2 + dy^2 <= floor(k^2 / 4), counted row by row.
constexpr uint32_t bokeh_disc_points(int k) {
    const int h = k / 2, q4 = (k * k) / 4;
    uint32_t n = 0;
    int w = h;
    for (int dy = 0; dy <= h; dy++) {
        while (w * w > q4 - dy * dy) w--;                           // (q4 - dy^2 >= 0: h^2 <= q4)
        n += (dy ? 2u : 1u) * (uint32_t)(2 * w + 1);
    }
    return n;
}
struct BokehWeights { uint32_t wt[kBkCodes]; };
constexpr BokehWeights bokeh_weights() {
    BokehWeights t{};
    for (int k = 0; k <= kBkMaxK; k++) t.wt[k] = (1u << 30) / bokeh_disc_points(k);
    t.wt[kBkMaxK + 1] = 0;
    return t;
}
static_assert(bokeh_disc_points(0) == 1 && bokeh_disc_points(1) == 1 && bokeh_disc_points(2) == 5 && bokeh_disc_points(127) == 12645, "N(k) of the header");
static_assert(bokeh_weights().wt[127] == 84914 && bokeh_weights().wt[0] == (1u << 30), "wt[k] of the header");
__constant__ BokehWeights g_bokeh_weights = bokeh_weights();

// HMAX: the largest h = K / 2 the LDS array has a halo for; NW: waves per workgroup.
template <int HMAX, int NW>
__global__ __launch_bounds__(64 * NW) void k_bokeh(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                   uint8_t *__restrict__ art, size_t ap, int rows, int cols, int kernelSize, float focus,
                                                   const float *__restrict__ focus_px) {
    constexpr int P = kBkW + 2 * HMAX;                               // words per LDS row
    __shared__ uint32_t Ws[(kBkH + 2 * HMAX) * P];                   // Ws[(HMAX + ty) * P + HMAX + tx] = the word of pixel (x0 + tx, y0 + ty)
    __shared__ uint32_t wts[kBkCodes];
    __shared__ int wmax[NW];                                         // the largest |s| each wave staged
    static_assert(sizeof(Ws) + sizeof(wts) + sizeof(wmax) <= 160 * 1024 && NW <= kBkH && kBkH % NW == 0 && 64 * NW >= kBkCodes,
                  "the tile with its halo fits a CU's LDS; every wave walks the same number of rows; a thread per weight");
    const int h = kernelSize >> 1;                                   // <= HMAX (launch_bokeh)
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * kBkW, y0 = blockIdx.y * kBkH;
    const float f = clamp_depth(focal_depth(focus, focus_px));
    const float Kf = (float)kernelSize;

    // staging: rows y0 - h .. y0 + 15 + h, columns x0 - h .. x0 + 63 + h; a wave a row at a time, its lanes consecutive words
    if (threadIdx.x < kBkCodes) wts[threadIdx.x] = g_bokeh_weights.wt[threadIdx.x];
    const int rw = kBkW + 2 * h, rh = kBkH + 2 * h;
    int kmax = 0;
    for (int ry = wave; ry < rh; ry += NW) {
        const int gy = y0 - h + ry;
        const bool row_inside = (unsigned)gy < (unsigned)rows;       // (wave-uniform)
        const float *drow = (const float *)((const char *)depth + (size_t)(row_inside ? gy : 0) * dp);
        const uint8_t *orow = orig + (size_t)(row_inside ? gy : 0) * op;
        uint32_t *wrow = Ws + (HMAX - h + ry) * P + (HMAX - h);
        for (int rx = lane; rx < rw; rx += 64) {
            const int gx = x0 - h + rx;
            uint32_t word = kBkOutside;
            if (row_inside && (unsigned)gx < (unsigned)cols) {
                const float t = clamp_depth(drow[gx]) - f;
                const int k = (int)((double)(Kf * fabsf(t)) / 255.0);             // 0 .. K: |t| <= 255
                const int s = t < 0.0f ? -k : k;
                kmax = max(kmax, k);
                word = load_bgr(orow + 3 * (size_t)gx) | ((uint32_t)(s & 255) << 24);
            }
            wrow[rx] = word;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) kmax = max(kmax, __shfl_xor(kmax, m));
    if (lane == 0) wmax[wave] = kmax;
    __syncthreads();                                                 // the one barrier: every wave reaches it

    int hw = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) hw = max(hw, wmax[i]);
    hw = __builtin_amdgcn_readfirstlane(hw);                         // the largest |s| of the tile and its halo
    const int hh = min(hw >> 1, h), q4 = (hw * hw) >> 2;             // the window: the disc of diameter hw (hh^2 <= q4)

    for (int ty = wave; ty < kBkH; ty += NW) {
        const int x = x0 + lane, y = y0 + ty;
        if (y >= rows) break;                                        // wave-uniform (behind the barrier)
        const uint32_t *own = Ws + (HMAX + ty) * P + HMAX + lane;
        const uint32_t wp = *own;                                    // the outside code beyond the image (such a lane stores nothing)
        uint32_t res = wp;                                           // no |s| > 1 staged: the original
        if (hw > 1) {
            const int sp = (int)wp >> 24, kp = abs(sp);
            u64 W = 0, Sb = 0, Sg = 0, Sr = 0;
            int wd = 0;                                              // isqrt(q4 - dy^2), carried from row to row
            for (int dy = -hh; dy <= hh; dy++) {
                const int n = q4 - dy * dy;                          // >= 0
                while ((wd + 1) * (wd + 1) <= n) wd++;
                while (wd * wd > n) wd--;
                const uint32_t *rp = own + dy * P;
                const int dy4 = 4 * dy * dy;
#pragma unroll 4
                for (int dx = -wd; dx <= wd; dx++) {                 // (wd <= hh <= h: inside the staged region)
                    const uint32_t w = rp[dx];
                    const int d2 = dy4 + 4 * dx * dx;                // (wave-uniform)
                    const int sq = (int)w >> 24, kq = abs(sq);
                    const int ke = sq > sp ? min(kq, kp) : kq;
                    const uint32_t wgt = wts[__mul24(ke, ke) >= d2 ? ke : kBkMaxK + 1];      // (an unconditional read: wt[128] == 0)
                    W += wgt;
                    Sb += (u64)wgt * (w & 255u); Sg += (u64)wgt * ((w >> 8) & 255u); Sr += (u64)wgt * ((w >> 16) & 255u);
                }
            }
            if (x < cols) res = (uint32_t)(Sb / W) | ((uint32_t)(Sg / W) << 8) | ((uint32_t)(Sr / W) << 16);      // W >= wt[kp] > 0: p reaches itself
        }
        if (x < cols) store_bgr(art + (size_t)y * ap + 3 * (size_t)x, res);
    }
}

template <int HMAX, int NW>
static void launch_class(rtdd_ctx *ctx, const Effect &e, const float *focus_px) {
    const dim3 g((e.cols + kBkW - 1) / kBkW, (e.rows + kBkH - 1) / kBkH);
    hipLaunchKernelGGL((k_bokeh<HMAX, NW>), g, dim3(64 * NW), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic,
                       e.artisticPitch, e.rows, e.cols, e.kernelSize, e.focusDepth, focus_px);
}

// rtdd_simulate_bokeh (arguments checked by effects_api.cpp): one launch.  The class is the smallest whose halo holds K / 2.
int launch_bokeh(rtdd_ctx *ctx, const Effect &e) {
    if (e.kernelSize < 0 || e.kernelSize > kBkMaxK) return fail(ctx, RTDD_ERR_INVALID, "bokeh: window scale outside [0, 127]");
    const float *focus_px = pixel_ptr(e.depth, e.depthPitch, e.focusX, e.focusY);      // the pixel form of the focus
    const int h = e.kernelSize / 2;
    if (h <= 8) launch_class<8, 4>(ctx, e, focus_px);
    else if (h <= 16) launch_class<16, 4>(ctx, e, focus_px);
    else if (h <= 32) launch_class<32, 8>(ctx, e, focus_px);
    else launch_class<63, 16>(ctx, e, focus_px);
    RTDD_LAUNCH_CHECK(ctx, "k_bokeh");
    return RTDD_OK;
}

}  // namespace rtdd
