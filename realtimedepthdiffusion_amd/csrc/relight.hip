// relight.hip -- depth-aware relighting (rtdd_simulate_relight, include/rtdd.h): the depth map read as a surface, shaded by a
// directional or a point light.  The first effect here that needs a depth NEIGHBOURHOOD: the central difference of the clamped depth.
//
// A stream like haze_ex (3 B + 4 B read, 3 B written per pixel): a lane takes FOUR pixels of a row -- the image as three dwords in and
// out, the depth as one float4 -- a wave 256 pixels of one row, a workgroup four rows.  The left / right depth neighbours of a lane's
// four pixels are its neighbour lanes' outer depths (ds_bpermute; lanes 0 and 63 load theirs), the rows above and below are read again
// as float4 (the workgroup's own rows and its neighbours': cache hits).  Rows that are not aligned for that take one pixel per lane
// with the same arithmetic.  No LDS, no atomics.
//
// The arithmetic is the header's, operation by operation: this translation unit is compiled with -ffp-contract=off and holds no fmaf,
// `/` and sqrtf are the correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt), denormals are kept -- the bytes are those of
// tests/relight_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"
#include "relight_common.hpp"

namespace rtdd {

// VEC: four pixels per lane (rows of both images 4-byte aligned, rows of the depth map 16-byte aligned).
template <bool POINT, bool VEC>
__global__ __launch_bounds__(256) void k_relight(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                 uint8_t *__restrict__ art, size_t ap, int rows, int cols, Light L,
                                                 const float *__restrict__ anchor_px) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform: a wave is one row
    const int lane = threadIdx.x & 63;
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const float *urow = (const float *)((const char *)depth + (size_t)max(y - 1, 0) * dp);
    const float *lrow = (const float *)((const char *)depth + (size_t)min(y + 1, rows - 1) * dp);
    const uint8_t *orow = orig + (size_t)y * op;
    uint8_t *arow = art + (size_t)y * ap;
    const float Lz = POINT ? point_light_height(L, anchor_px) : 0.0f;
    // one pixel, every neighbour from memory: the one-pixel-per-lane path and the ragged end of a vectorised row
    auto pixel = [&](int x) {
        float dc;
        const float s = shade_in_rows<POINT>(L, Lz, drow, urow, lrow, cols, x, y, dc);     // (the wave's rows: the vectorised path reads them too)
#pragma unroll
        for (int c = 0; c < 3; c++) arow[3 * (size_t)x + c] = (uint8_t)relight_u8(L, c, L.ambient, s, orow[3 * (size_t)x + c]);
    };
    if (!VEC) {
        const int x = blockIdx.x * 64 + lane;
        if (x < cols) pixel(x);
        return;
    }
    const int x = (blockIdx.x * 64 + lane) * 4;
    const bool whole = x + 3 < cols;
    // the lane's own depths; a lane at or beyond the ragged end holds the row's last depth in .x: what its left neighbour lane wants
    float4 c4 = {0.0f, 0.0f, 0.0f, 0.0f}, u4 = c4, l4 = c4;
    raw12 o = {0u, 0u, 0u};
    if (whole) {
        c4 = *(const float4 *)(drow + x); u4 = *(const float4 *)(urow + x); l4 = *(const float4 *)(lrow + x);
        o = load_raw<true>(orow, x, cols);
    } else {
        c4.x = drow[min(x, cols - 1)];
    }
    // d(x - 1) and d(x + 4), replicated at the borders: the neighbour lanes' outer depths; the wave's two edge lanes load theirs
    float left = __shfl_up(c4.w, 1), right = __shfl_down(c4.x, 1);
    if (lane == 0) left = drow[min(max(x - 1, 0), cols - 1)];
    if (lane == 63) right = drow[min(x + 4, cols - 1)];
    if (!whole) {
        for (int xx = x; xx < cols; xx++) pixel(xx);
        return;
    }
    const float dv[6] = {clamp_depth(left), clamp_depth(c4.x), clamp_depth(c4.y), clamp_depth(c4.z), clamp_depth(c4.w), clamp_depth(right)};
    const float uv[4] = {u4.x, u4.y, u4.z, u4.w}, lv[4] = {l4.x, l4.y, l4.z, l4.w};
    uint32_t ob[12], rb[12];
    bytes12(o, ob);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float s = relight_shade<POINT>(L, Lz, dv[i + 1], dv[i], dv[i + 2], clamp_depth(uv[i]), clamp_depth(lv[i]), x + i, y);
#pragma unroll
        for (int c = 0; c < 3; c++) rb[3 * i + c] = relight_u8(L, c, L.ambient, s, ob[3 * i + c]);
    }
    store_bytes12(arow + 3 * (size_t)x, rb);
}

// rtdd_simulate_relight (arguments checked and the light prepared by effects_api.cpp): one launch.
int launch_relight(rtdd_ctx *ctx, const Effect &e) {
    const Light &L = e.light;
    const bool point = L.kind == RTDD_LIGHT_POINT;
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, L.anchorX, L.anchorY) : nullptr;     // the pixel form of the anchor's depth
    const bool vec = rows_aligned(e.original, e.originalPitch) && rows_aligned(e.artistic, e.artisticPitch) && rows_aligned(e.depth, e.depthPitch, 16);
    const dim3 g((e.cols + (vec ? 255 : 63)) / (vec ? 256 : 64), (e.rows + 3) / 4);
#define RTDD_RL_LAUNCH(P, V) hipLaunchKernelGGL((k_relight<P, V>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols, L, anchor_px)
    if (point) { if (vec) RTDD_RL_LAUNCH(true, true); else RTDD_RL_LAUNCH(true, false); }
    else { if (vec) RTDD_RL_LAUNCH(false, true); else RTDD_RL_LAUNCH(false, false); }
#undef RTDD_RL_LAUNCH
    RTDD_LAUNCH_CHECK(ctx, "k_relight");
    return RTDD_OK;
}

}  // namespace rtdd
