// paint_common.hpp -- what the two annotation painters, k_paint_strokes<> (image_kernels.hip) and k_fill_polygon (fill_polygon.hip), and
// their launchers share: the tile, the packed points, the quotient of the ramp's label rule and the launch box.  Included inside no
// namespace; everything here is in namespace rtdd.
#pragma once

#include <algorithm>

#include "rtdd_internal.hpp"

namespace rtdd {

// A workgroup owns a 64 x 16 tile of the launch box: 256 threads, one wave per row and four rows per wave.
constexpr int kPaintTileW = 64, kPaintTileH = 16;

// a point as one word: x | y << 16, two's complement halves (coordinates in [-32768, 32767])
static inline uint32_t pack_xy(int x, int y) { return ((uint32_t)x & 0xFFFFu) | ((uint32_t)y << 16); }
__device__ __forceinline__ int unpack_x(uint32_t p) { return (int16_t)(p & 0xFFFF); }
__device__ __forceinline__ int unpack_y(uint32_t p) { return (int16_t)(p >> 16); }

// The label of a ramp (include/rtdd.h, rtdd_paint_ramp_strokes): L = N div D with N = 2 (l0 (dd - t) + l1 t) + dd and D = 2 dd, t the
// pixel's projection on the segment clamped to [0, dd].  The callers form N and D, guarantee 0 <= N <= 511 dd < 2^45 and D < 2^36, and
// hand in the estimate y = ramp_f32(N) * v_rcp_f32((float)D) -- they differ in where the reciprocal comes from, and the product is
// theirs so that each kernel's order of evaluation stays what it was.
// The quotient x = N / D is known to lie in [0, 255.5], so the compiler's general 64-bit division is not needed: an f32 estimate and one
// correction step.  fn and fd are N and D rounded to f32 (the high word of N is below 2^13 and exact, the low word and the sum round
// once each: relative error <= 2^-23; D likewise), v_rcp_f32 is good to 1 ulp (2^-23) and the product rounds once more (2^-24):
// y = fn * rcp(fd) = x (1 + e) with |e| < 2^-21, so |y - x| < 256 * 2^-21 = 2^-13 and q = trunc(y) >= 0 is floor(x) - 1, floor(x) or
// floor(x) + 1.  The remainder r = N - q D (|r| < 2 D < 2^37, exact in 64 bits) says which: r < 0: one too many; r >= D: one too few;
// afterwards 0 <= N - q D < D, which is the definition of N div D.
__device__ __forceinline__ float ramp_f32(long long N) { return __builtin_fmaf((float)(uint32_t)((unsigned long long)N >> 32), 4294967296.0f, (float)(uint32_t)N); }
__device__ __forceinline__ int ramp_quotient(long long N, long long D, float y) {
    int q = (int)y;
    const long long r = N - (long long)q * D;
    q += (int)(r >= D) - (int)(r < 0);
    return q;
}

// The launch over the inclusive box (x0, y0) .. (x1, y1): clipped to the image, x0 rounded down to a multiple of 64 (a wave's 64 pixels
// start on a 64-pixel boundary of the row), one workgroup per tile.  False: the box misses the image, nothing to do.
static inline bool paint_grid(int &x0, int &y0, int &x1, int &y1, int rows, int cols, dim3 &grid) {
    x0 = std::max(x0, 0); y0 = std::max(y0, 0); x1 = std::min(x1, cols - 1); y1 = std::min(y1, rows - 1);
    if (x1 < x0 || y1 < y0) return false;
    x0 &= ~63;
    grid = dim3((x1 - x0) / kPaintTileW + 1, (y1 - y0) / kPaintTileH + 1);
    return true;
}

}  // namespace rtdd
