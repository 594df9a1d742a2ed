// relight_shadow.hip -- relighting with cast shadows (rtdd_simulate_relight_shadowed, include/rtdd.h): k_relight's shade, and per pixel a
// march over the height field H = relief * (255 - d') towards the light.  One launch renders shade and shadow together.
//
// One pixel per lane, a wave 64 pixels of one row, a workgroup four rows.  The lanes of a wave step together, so what a wave reads at
// step k is one run of 64 consecutive heights of one row (a directional light: every lane has the same offset; a point light: nearly
// so) -- one or two cache lines per step, shared with the waves above and below.  Leaving the image is monotonic in k, so every lane
// first bounds its steps to those inside the image; the march itself tests no bounds.  The steps are taken FOUR at a time: the four
// addresses depend on nothing read before, so their loads are in flight together and the exits are tested once per group.  That is
// allowed because q is a maximum: the order of the steps does not matter, and a group that reaches past the last step repeats it.  The
// exits are the header's two: q == 1, and for rise >= 0 a ray above relief * 255.  A wave runs as long as its longest ray.  No LDS, no
// atomics.
//
// The arithmetic is the header's, operation by operation: compiled like relight.hip with -ffp-contract=off, no fmaf, the correctly
// rounded `/` and sqrtf, denormals kept -- the bytes are those of tests/shadow_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"
#include "relight_common.hpp"

namespace rtdd {

template <bool POINT, bool SOFT>
__global__ __launch_bounds__(256) void k_relight_shadow(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                        uint8_t *__restrict__ art, size_t ap, int rows, int cols, Light L, Shadow S,
                                                        const float *__restrict__ anchor_px) {
    const int y = blockIdx.y * 4 + wave_id();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (y >= rows || x >= cols) return;                              // (no cross-lane operation below)
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const float Lz = POINT ? point_light_height(L, anchor_px) : 0.0f;
    float dc;
    const float shade = shade_at<POINT>(L, Lz, depth, dp, rows, cols, x, y, dc);
    const float h = L.relief * (255.0f - dc);                        // H(x, y)
    const float q = shadow_march<POINT, SOFT ? 1 : 0>(L, S, Lz, h, drow, dp, x, y, rows, cols);
    const float lit = shade * (1.0f - (S.strength * q));
    const uint8_t *o = orig + (size_t)y * op + 3 * (size_t)x;
    uint8_t *a = art + (size_t)y * ap + 3 * (size_t)x;
#pragma unroll
    for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8(L, c, L.ambient, lit, o[c]);
}

// rtdd_simulate_relight_shadowed (arguments checked, the light and the direction prepared by effects_api.cpp): one launch.  Where no pixel can
// be shadowed (shadow_cannot_show) the launch is k_relight's own.
int launch_relight_shadow(rtdd_ctx *ctx, const Effect &e) {
    const Light &L = e.light;
    const Shadow &S = e.shadow;
    const bool point = L.kind == RTDD_LIGHT_POINT;
    if (shadow_cannot_show(L, S)) return launch_relight(ctx, e);
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, L.anchorX, L.anchorY) : nullptr;
    const bool soft = S.softness > 0.0f;
    const dim3 g((e.cols + 63) / 64, (e.rows + 3) / 4);
#define RTDD_RS_LAUNCH(P, F) hipLaunchKernelGGL((k_relight_shadow<P, F>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols, L, S, anchor_px)
    if (point) { if (soft) RTDD_RS_LAUNCH(true, true); else RTDD_RS_LAUNCH(true, false); }
    else { if (soft) RTDD_RS_LAUNCH(false, true); else RTDD_RS_LAUNCH(false, false); }
#undef RTDD_RS_LAUNCH
    RTDD_LAUNCH_CHECK(ctx, "k_relight_shadow");
    return RTDD_OK;
}

}  // namespace rtdd
