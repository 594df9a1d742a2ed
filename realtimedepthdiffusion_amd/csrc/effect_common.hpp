// effect_common.hpp -- what the depth-effect translation units (effect_kernels.hip, lens_blur.hip, relight.hip, relight_shadow.hip,
// parallax.hip, ambient_occlusion.hip, lighting.hip, bokeh.hip, composite.hip, remove.hip) and relight_common.hpp share.
// Device: the clamped depth, the loads and stores of a BGR pixel packed b | g << 8 | r << 16, the packed 3 x 21-bit pixel sums of the
// defocus tables, the 64-bit DPP scans, the quotients, the focus read, the workgroup -> tile decode, the tile geometry.  Host: the pixel
// form, row alignment, the launch grids of the two tile kernels and the two table lookups, the table buffer.
// Included inside no namespace; everything here is in namespace rtdd.
#pragma once

#include "rtdd_internal.hpp"

namespace rtdd {

// ---- the clamped depth, and a BGR pixel as b | g << 8 | r << 16 ----
__device__ __forceinline__ float clamp_depth(float d) { return fminf(fmaxf(d, 0.0f), 255.0f); }     // a NaN depth is 0 (stereo's clamp)
// rtdd_remove_object's and rtdd_fill_surface's d': NaN, -0 and every negative are +0, so equal bits are equal depths
__device__ __forceinline__ float remove_depth(float d) { return d > 0.0f ? fminf(d, 255.0f) : 0.0f; }

__device__ __forceinline__ uint32_t load_bgr(const uint8_t *px) { return (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16); }
__device__ __forceinline__ void store_bgr(uint8_t *px, uint32_t v) { px[0] = (uint8_t)v; px[1] = (uint8_t)(v >> 8); px[2] = (uint8_t)(v >> 16); }
// four pixels (each < 2^24) as the three dwords at px, the first of the four (4-byte aligned)
__device__ __forceinline__ void store_bgr4(uint8_t *px, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) {
    uint32_t *a3 = (uint32_t *)px;
    a3[0] = o0 | (o1 << 24);
    a3[1] = (o1 >> 8) | (o2 << 16);
    a3[2] = (o2 >> 16) | (o3 << 8);
}
// a wave's 64 pixels `res` of columns x0 .. x0 + 63 of the row `arow` (4-byte aligned, all 64 inside the image) as dwords: the three
// dwords of a quad of pixels stored by its first three lanes after one quad permute
__device__ __forceinline__ void store_bgr_quads(uint8_t *arow, int x0, int lane, uint32_t res) {
    const int j = lane & 3;
    const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)res, 0xF9, 0xF, 0xF, true);   // quad_perm:[1,2,3,3]
    const uint32_t out = (res >> (8 * j)) | (nxt << ((24 - 8 * j) & 31));
    if (j < 3) ((uint32_t *)(arow + 3 * (size_t)x0))[3 * (lane >> 2) + j] = out;
}

// ---- packed sums and scans (the summed-area table of effect_kernels.hip explains the packing) ----
typedef unsigned long long u64;
constexpr int kSatMaxArea = 8224;                                   // 8224 * 255 = 2 097 120 < 2^21
constexpr u64 kSatFieldMask = (1ull << 21) - 1;

__device__ __forceinline__ u64 pack_px(uint32_t b, uint32_t g, uint32_t r) { return (u64)(b | (g << 21)) | ((u64)(r << 10) << 32); }

// four interleaved BGR pixels held in three dwords -> four packed pixels
__device__ __forceinline__ void unpack4(uint32_t w0, uint32_t w1, uint32_t w2, u64 px[4]) {
    px[0] = pack_px(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255);
    px[1] = pack_px(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
    px[2] = pack_px((w1 >> 16) & 255, w1 >> 24, w2 & 255);
    px[3] = pack_px((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
}

// the twelve bytes of pixels x .. x+3 of an image row as three dwords (zero beyond `cols`); VEC: the row is 4-byte aligned
struct raw12 { uint32_t w0, w1, w2; };
template <bool VEC>
__device__ __forceinline__ raw12 load_raw(const uint8_t *__restrict__ row, int x, int cols) {
    raw12 v;
    if (VEC && x + 3 < cols) {
        const uint32_t *q = (const uint32_t *)(row + 3 * (size_t)x);
        v.w0 = q[0]; v.w1 = q[1]; v.w2 = q[2];
    } else {
        uint32_t w[3] = {0, 0, 0};
        const int n = 3 * min(max(cols - x, 0), 4);
        const uint8_t *q = row + 3 * (size_t)x;
#pragma unroll
        for (int i = 0; i < 12; i++) if (i < n) w[i >> 2] |= (uint32_t)q[i] << (8 * (i & 3));
        v.w0 = w[0]; v.w1 = w[1]; v.w2 = w[2];
    }
    return v;
}

// the same twelve bytes one per word, b[3 * i + c] = channel c of pixel i, and back: the three dwords stored at px, the first of the
// four pixels (4-byte aligned)
__device__ __forceinline__ void bytes12(const raw12 &v, uint32_t b[12]) {
#pragma unroll
    for (int i = 0; i < 4; i++) { b[i] = (v.w0 >> (8 * i)) & 255; b[4 + i] = (v.w1 >> (8 * i)) & 255; b[8 + i] = (v.w2 >> (8 * i)) & 255; }
}
__device__ __forceinline__ void store_bytes12(uint8_t *__restrict__ px, const uint32_t b[12]) {              // (every b[i] <= 255)
    uint32_t *a3 = (uint32_t *)px;
#pragma unroll
    for (int i = 0; i < 3; i++) a3[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
}

// the three fields of a packed sum X (each < 2^21: at most kSatMaxArea pixels) added to running channel sums
__device__ __forceinline__ void add_fields(u64 X, uint32_t &sb, uint32_t &sg, uint32_t &sr) {
    sb += (uint32_t)(X & kSatFieldMask); sg += (uint32_t)((X >> 21) & kSatFieldMask); sr += (uint32_t)(X >> 42);
}

#define RTDD_DPP64(src, ctrl, rows, banks)                                                                       \
    (((u64)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((src) >> 32), ctrl, rows, banks, true) << 32) | \
     (u64)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(src), ctrl, rows, banks, true))

// inclusive prefix sums of a 64-bit value by DPP (VALU only), each scan the one before plus a step: over the 16 lanes of each DPP row
// (the wave totals of a workgroup: at most 16), over the 32 lanes of each half of a wave, over the 64 lanes of a wave
__device__ __forceinline__ u64 row16_incl_scan64(u64 v) {
    u64 t = v + RTDD_DPP64(v, 0x111, 0xF, 0xF);         // row_shr:1
    t += RTDD_DPP64(v, 0x112, 0xF, 0xF);                // row_shr:2
    t += RTDD_DPP64(v, 0x113, 0xF, 0xF);                // row_shr:3   -> v[i-3..i] within a row of 16
    t += RTDD_DPP64(t, 0x114, 0xF, 0xE);                // row_shr:4, banks 1-3
    t += RTDD_DPP64(t, 0x118, 0xF, 0xC);                // row_shr:8, banks 2-3  -> prefix within each row of 16
    return t;
}
__device__ __forceinline__ u64 half_incl_scan64(u64 v) {
    const u64 t = row16_incl_scan64(v);
    return t + RTDD_DPP64(t, 0x142, 0xA, 0xF);          // row_bcast:15 into rows 1 and 3
}
__device__ __forceinline__ u64 wave_incl_scan64(u64 v) {
    const u64 t = half_incl_scan64(v);
    return t + RTDD_DPP64(t, 0x143, 0xC, 0xF);          // row_bcast:31 into rows 2 and 3
}
__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    return ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) | (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

struct alignas(16) u64x2 { u64 a, b; };

// (uchar)(sum / count) of src/GPUDepthEffect.cu:68-70 (f32 divide, truncation) for an exact integer sum s < 2^24 and count < 2^16: a
// non-integer quotient <= 255 is at least 1/count > 2^-16 below the next integer, more than the f32 half-ulp 2^-17 there, so the
// rounded quotient truncates to floor(s / count) -- computed with the shared reciprocal and one exact integer correction.
__device__ __forceinline__ uint32_t quot_u8(uint32_t s, uint32_t count, float rc) {
    int n = (int)((float)s * rc);
    const int rem = (int)s - n * (int)count;
    n += rem < 0 ? -1 : (rem >= (int)count ? 1 : 0);
    return (uint32_t)min(n, 255);
}

// The same three quotients, packed b | g << 8 | r << 16, in 8 instead of 14 instructions each: q = trunc(s * rlo) with rlo = RN(1 / c) less
// 2^-21 relative never exceeds floor(s / c) (v_rcp_f32 is within 1 ulp, the two products round by 2^-24 each) and is at most one below
// it (s / c < 256, 256 * 2^-20.5 < 1); the remainder s - q c -- one fma, exact: an integer in [0, 2 c) -- says which; v_cvt_pk_u8_f32
// places the byte (and saturates what a depth that is no depth produces).
__device__ __forceinline__ uint32_t quot3_u8(uint32_t sb, uint32_t sg, uint32_t sr, uint32_t count, float rc) {
    const float cf = (float)count, rlo = rc * (1.0f - 0x1p-21f);
    auto q1 = [&](uint32_t s) {
        const float sf = (float)s, q = __builtin_truncf(sf * rlo), r = __builtin_fmaf(-q, cf, sf);
        return r >= cf ? q + 1.0f : q;
    };
    uint32_t out = __builtin_amdgcn_cvt_pk_u8_f32(q1(sb), 0, 0u);
    out = __builtin_amdgcn_cvt_pk_u8_f32(q1(sg), 1, out);
    return __builtin_amdgcn_cvt_pk_u8_f32(q1(sr), 2, out);
}

// the reference's float -> uchar cast with its out-of-range cases defined: saturate, then truncate
__device__ __forceinline__ uint32_t store_u8(float v) {
    if (!(v >= 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint32_t)(int)v;
}

// The three quotients b | g << 8 | r << 16 of channel sums that a wave took from the image (cnt >= 1 pixels): exact integer quotients on
// quot_u8's domain, cnt < 2^16 and sums < 2^24 -- every window of a depth map -- and beyond it (an out-of-range depth) the reference's
// own f32 divide of its f32 sums, which round there.
__device__ __forceinline__ uint32_t quot3_exact_or_f32(uint32_t sb, uint32_t sg, uint32_t sr, uint32_t cnt) {
    if (cnt < 65536u && (sb | sg | sr) < (1u << 24)) {
        const float rc = __builtin_amdgcn_rcpf((float)cnt);
        return quot_u8(sb, cnt, rc) | (quot_u8(sg, cnt, rc) << 8) | (quot_u8(sr, cnt, rc) << 16);
    }
    const float count = (float)cnt;
    return store_u8((float)sb / count) | (store_u8((float)sg / count) << 8) | (store_u8((float)sr / count) << 16);
}

// FOCUS (rtdd_simulate_refocus): the window is sized by |depth - f| instead of depth, f = *focus_px (one uniform load per wave: the
// depth map's value at the focus pixel, read when the kernel runs) or, focus_px == nullptr, the value `focus`.  Nothing else changes.
__device__ __forceinline__ float focal_depth(float focus, const float *__restrict__ focus_px) {
    return focus_px ? *focus_px : focus;
}

// ---- workgroup -> tile (k_defocus, k_lens_gather and the two LDS kernels) ----
// The tile of workgroup p, which the dispatcher places on XCD p % 8: each XCD takes xcd_tiles consecutive tiles, a band of tile ROWS
// (xcd_tiles == 0: tile p).  The caller leaves if it is >= ntiles, before it divides anything.
__device__ __forceinline__ int band_tile(int p, int xcd_tiles) { return xcd_tiles > 0 ? (p & 7) * xcd_tiles + (p >> 3) : p; }
// Tile (tx, ty) of workgroup p of a table lookup: band_tile, or (strip_w > 0) each XCD takes a COLUMN strip strip_w tiles wide and walks
// it row by row.  false: a workgroup beyond the tiles (workgroup-uniform).
__device__ __forceinline__ bool tile_of_workgroup(int p, int gx, int ntiles, int xcd_tiles, int strip_w, int &tx, int &ty) {
    if (strip_w > 0) {
        const int q = p >> 3;
        tx = (p & 7) * strip_w + q % strip_w; ty = q / strip_w;
        if (tx >= gx || ty * gx >= ntiles) return false;
    } else {
        const int tile = band_tile(p, xcd_tiles);
        if (tile >= ntiles) return false;
        tx = tile % gx; ty = tile / gx;
    }
    return true;
}

// ---- the tile of the LDS kernels (k_defocus_tile, k_lens_tile) ----
constexpr int kDtW = 64, kDtHM = 28, kDtRW = 124, kDtWorkers = 8;
static_assert(kDtW + 2 * kDtHM + 3 <= kDtRW && kDtRW % 4 == 0 && kDtRW / 4 <= 32, "the region: tile + both margins + the alignment of its first column, one group of four per lane of a half-wave");

// ---- host: what the launchers share ----
// The pixel form of a depth-valued argument: the address of depth(x, y), which the kernel reads when it runs (no host synchronisation; a
// heal's replay reads it again).  x < 0: the value form, nullptr.
inline const float *pixel_ptr(const float *depth, size_t pitch, int x, int y) {
    return x >= 0 ? (const float *)((const char *)depth + (size_t)y * pitch) + x : nullptr;
}
// every row of an image starts at a multiple of `a` bytes -- what the kernels' VEC paths ask for: 4 for dword accesses to the u8 images,
// 16 for a float4 of depth
inline bool rows_aligned(const void *p, size_t pitch, size_t a = 4) { return (uintptr_t)p % a == 0 && pitch % a == 0; }

// the context's table buffer (ctx->sat), grown to `words` u32 words; a new buffer holds no table geometry
inline int ensure_sat(rtdd_ctx *ctx, size_t words) {
    if (ctx->sat_elems < words) {
        if (ctx->sat) { RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream)); RTDD_HIP(ctx, hipFree(ctx->sat)); ctx->sat = nullptr; ctx->sat_elems = 0; }
        RTDD_HIP(ctx, hipMalloc((void **)&ctx->sat, words * sizeof(uint32_t)));
        ctx->sat_elems = words; ctx->sat_rows = ctx->sat_cols = 0;
    }
    return RTDD_OK;
}

// The launch of an LDS-tile kernel: tiles of 64 x 16 where all of those are resident at once (`low`), else of 64 x 24; from 64 tiles on
// each XCD takes xcd_tiles consecutive ones (tile_of_workgroup).
struct DtGrid { int gx, ntiles, xcd_tiles; bool low; dim3 grid; };
inline DtGrid dt_grid(const rtdd_ctx *ctx, int rows, int cols) {
    DtGrid t;
    t.gx = (cols + kDtW - 1) / kDtW;
    t.low = t.gx * ((rows + 15) / 16) <= 2 * ctx->num_cus;
    const int th = t.low ? 16 : 24;
    t.ntiles = t.gx * ((rows + th - 1) / th);
    t.xcd_tiles = t.ntiles >= 64 ? (t.ntiles + 7) / 8 : 0;
    t.grid = dim3(t.xcd_tiles > 0 ? 8 * t.xcd_tiles : t.ntiles);
    return t;
}

// The launch of a table lookup (k_defocus, k_lens_gather) over out_rows rows: workgroups of 64 columns x wg_rows rows.  Column strips
// per XCD where the table rows between a window's bottom and top edge (2 * reach rows of row_bytes), over the whole image width, outgrow
// an XCD's L2 (RTDD_OPT_DEFOCUS_STRIPS: 0 this rule, 1 never, 2 always; measured in profiles/r06_defocus_strips.txt).
struct LookupGrid { int gx, ntiles, xcd_tiles, strip_w; dim3 grid; };
inline LookupGrid lookup_grid(const rtdd_ctx *ctx, int out_rows, int cols, int wg_rows, int reach, size_t row_bytes) {
    LookupGrid t;
    t.gx = (cols + 63) / 64;
    const int gy = (out_rows + wg_rows - 1) / wg_rows;
    t.ntiles = t.gx * gy;
    t.xcd_tiles = t.ntiles >= 64 ? (t.ntiles + 7) / 8 : 0;
    const bool strips = ctx->opt.defocus_strips == 2 || (ctx->opt.defocus_strips == 0 && (size_t)2 * reach * row_bytes > ((size_t)3 << 20) && t.gx >= 16);
    t.strip_w = strips ? (t.gx + 7) / 8 : 0;
    t.grid = dim3(t.strip_w > 0 ? 8 * t.strip_w * gy : t.xcd_tiles > 0 ? 8 * t.xcd_tiles : t.ntiles);
    return t;
}

}  // namespace rtdd
