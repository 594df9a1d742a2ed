// effect_common.hpp -- device helpers shared by the depth-effect translation units (effect_kernels.hip, lens_blur.hip): the packed
// 3 x 21-bit pixel sums of the defocus tables, the 64-bit DPP scans, the exact integer quotients, the focus read, the tile geometry.
// Included inside no namespace; everything here is in namespace rtdd.
#pragma once

#include "rtdd_internal.hpp"

namespace rtdd {

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

#define RTDD_DPP64(src, ctrl, rows, banks)                                                                       \
    (((u64)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((src) >> 32), ctrl, rows, banks, true) << 32) | \
     (u64)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(src), ctrl, rows, banks, true))

// inclusive prefix sum of a 64-bit value over the 64 lanes of a wave (the 7-step DPP scan: VALU only)
__device__ __forceinline__ u64 wave_incl_scan64(u64 v) {
    u64 t = v + RTDD_DPP64(v, 0x111, 0xF, 0xF);         // row_shr:1
    t += RTDD_DPP64(v, 0x112, 0xF, 0xF);                // row_shr:2
    t += RTDD_DPP64(v, 0x113, 0xF, 0xF);                // row_shr:3   -> v[i-3..i] within a row of 16
    t += RTDD_DPP64(t, 0x114, 0xF, 0xE);                // row_shr:4, banks 1-3
    t += RTDD_DPP64(t, 0x118, 0xF, 0xC);                // row_shr:8, banks 2-3  -> prefix within each row of 16
    t += RTDD_DPP64(t, 0x142, 0xA, 0xF);                // row_bcast:15 into rows 1 and 3
    t += RTDD_DPP64(t, 0x143, 0xC, 0xF);                // row_bcast:31 into rows 2 and 3
    return t;
}
// ... over the 16 lanes of each DPP row only (the wave totals of a workgroup: at most 16)
__device__ __forceinline__ u64 row16_incl_scan64(u64 v) {
    u64 t = v + RTDD_DPP64(v, 0x111, 0xF, 0xF);
    t += RTDD_DPP64(v, 0x112, 0xF, 0xF);
    t += RTDD_DPP64(v, 0x113, 0xF, 0xF);
    t += RTDD_DPP64(t, 0x114, 0xF, 0xE);
    t += RTDD_DPP64(t, 0x118, 0xF, 0xC);
    return t;
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

// FOCUS (rtdd_simulate_refocus): the window is sized by |depth - f| instead of depth, f = *focus_px (one uniform load per wave: the
// depth map's value at the focus pixel, read when the kernel runs) or, focus_px == nullptr, the value `focus`.  Nothing else changes.
__device__ __forceinline__ float focal_depth(float focus, const float *__restrict__ focus_px) {
    return focus_px ? *focus_px : focus;
}

// ---- the tile of the LDS kernels (k_defocus_tile, k_lens_tile) ----
constexpr int kDtW = 64, kDtHM = 28, kDtRW = 124, kDtWorkers = 8;
static_assert(kDtW + 2 * kDtHM + 3 <= kDtRW && kDtRW % 4 == 0 && kDtRW / 4 <= 32, "the region: tile + both margins + the alignment of its first column, one group of four per lane of a half-wave");

// inclusive prefix sum over the 32 lanes of each half of a wave (the wave scan without its last step)
__device__ __forceinline__ u64 half_incl_scan64(u64 v) {
    u64 t = v + RTDD_DPP64(v, 0x111, 0xF, 0xF);
    t += RTDD_DPP64(v, 0x112, 0xF, 0xF);
    t += RTDD_DPP64(v, 0x113, 0xF, 0xF);
    t += RTDD_DPP64(t, 0x114, 0xF, 0xE);
    t += RTDD_DPP64(t, 0x118, 0xF, 0xC);
    t += RTDD_DPP64(t, 0x142, 0xA, 0xF);                // row_bcast:15 into rows 1 and 3
    return t;
}

}  // namespace rtdd
