// lighting.hip -- the whole lighting model in one launch (rtdd_simulate_lighting, include/rtdd.h): k_relight's shade, k_relight_shadow's
// march towards the light and k_ambient_occlusion's horizons, per pixel:  out_c = o_c * ((ambient * ao) + (k_c * (shade * vis))).
// Every pixel is written once, `original` is read once, the shade is computed once.
//
// The shape is k_ambient_occlusion's (ambient_occlusion.hip): a workgroup owns a tile of 64 x 16 pixels and stages H = relief * (255 - d')
// ONCE in LDS for the tile and a halo of `radius` pixels, minus infinity outside the image; one barrier that every wave reaches; then
// a wave takes a row of the tile and its lanes 64 consecutive x.  Per row the horizons come from LDS exactly as there, and then every
// lane marches towards the light exactly as in k_relight_shadow (relight_shadow.hip): the steps bounded to those inside the image
// first, taken four at a time, the two exits of the header.  The march takes its samples from GLOBAL memory, not from the staged
// heights: it runs up to 1024 steps in an arbitrary direction and leaves any halo, so a march from LDS needs a second, global loop
// behind a per-lane switch; the one loop is what k_relight_shadow is measured with ("Full lighting").
//
// Template parameters, and why: RMAX / NW, the LDS array and the workgroup of the radius class (8, 16, 32, 64: k_ambient_occlusion's
// four, sized alike); DIRS, 4 or 8, the unrolled directions; POINT, the light's kind, which changes the shade and the direction of the
// march.  Hard or soft shadows are NOT a parameter: softness is wave-uniform, so the penumbra's division sits behind a scalar branch.
// 16 instantiations.  A term that is disabled is not rendered here at all: the launcher hands the call to the kernel of what is left.
//
// The arithmetic is the header's, operation by operation: compiled like relight.hip with -ffp-contract=off, no fmaf, the correctly
// rounded `/` and sqrtf, denormals kept -- the bytes are those of tests/lighting_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"
#include "relight_common.hpp"

namespace rtdd {

template <int RMAX, int NW, int DIRS, bool POINT>
__global__ __launch_bounds__(64 * NW) void k_lighting(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                      uint8_t *__restrict__ art, size_t ap, int rows, int cols, Light L, Shadow S, Occlusion A,
                                                      AoTables T, const float *__restrict__ anchor_px) {
    constexpr int P = kAoW + 2 * RMAX;                               // words per LDS row
    __shared__ float Hs[(kAoH + 2 * RMAX) * P];                      // Hs[(RMAX + ty) * P + RMAX + tx] = H(x0 + tx, y0 + ty)
    static_assert(sizeof(Hs) <= 160 * 1024 && NW <= kAoH && kAoH % NW == 0, "the tile with its halo fits a CU's LDS; every wave walks the same number of rows");
    const int r = A.radius;                                          // 1 .. RMAX (launch_lighting)
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * kAoW, y0 = blockIdx.y * kAoH;
    ao_stage<RMAX, NW>(Hs, depth, dp, rows, cols, x0, y0, r, A.relief, wave, lane);
    __syncthreads();                                                 // the one barrier: every wave reaches it

    const float Lz = POINT ? point_light_height(L, anchor_px) : 0.0f;
    for (int ty = wave; ty < kAoH; ty += NW) {
        const int x = x0 + lane, y = y0 + ty;
        const float *own = Hs + (RMAX + ty) * P + RMAX + lane;
        const float h = *own;                                        // H(x, y); minus infinity beyond the image (such a lane stores nothing)

        const float ao = ao_factor<RMAX, DIRS>(own, h, A, T, r);     // the horizons over the staged heights
        if (x >= cols || y >= rows) continue;                        // (behind the barrier; no cross-lane operation below)
        // The shade from the map itself, and the march towards the light: its steps bounded to those inside the IMAGE (not the staged
        // region), its samples from global memory
        float dc;
        const float shade = shade_at<POINT>(L, Lz, depth, dp, rows, cols, x, y, dc);
        const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
        const float q = shadow_march<POINT, kSoftByRecord>(L, S, Lz, h, drow, dp, x, y, rows, cols);
        const float lit = shade * (1.0f - (S.strength * q));
        const float amb = L.ambient * ao;
        const uint8_t *o = orig + (size_t)y * op + 3 * (size_t)x;
        uint8_t *a = art + (size_t)y * ap + 3 * (size_t)x;
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8(L, c, amb, lit, o[c]);
    }
}

template <int RMAX, int NW>
static void launch_class(rtdd_ctx *ctx, const Effect &e, const AoTables &T, const float *anchor_px) {
    const dim3 g((e.cols + kAoW - 1) / kAoW, (e.rows + kAoH - 1) / kAoH);
#define RTDD_LT_LAUNCH(D, PT) hipLaunchKernelGGL((k_lighting<RMAX, NW, D, PT>), g, dim3(64 * NW), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols, e.light, e.shadow, e.occlusion, T, anchor_px)
    if (e.light.kind == RTDD_LIGHT_POINT) { if (e.occlusion.directions == 4) RTDD_LT_LAUNCH(4, true); else RTDD_LT_LAUNCH(8, true); }
    else { if (e.occlusion.directions == 4) RTDD_LT_LAUNCH(4, false); else RTDD_LT_LAUNCH(8, false); }
#undef RTDD_LT_LAUNCH
}

// rtdd_simulate_lighting (arguments checked, the light, the march and the occlusion prepared by effects_api.cpp): one launch.  A term
// that cannot show costs nothing: without occlusion (no radius, no strength, a flat surface: ao == 1) the launch is
// k_relight_shadow's own, which without shadows is k_relight's; without shadows (no steps, no strength, a directional light straight
// above: vis == 1) it is k_ambient_occlusion's under the light.
int launch_lighting(rtdd_ctx *ctx, const Effect &e) {
    static const AoTables T = ao_tables();
    const Light &L = e.light;
    const Shadow &S = e.shadow;
    const Occlusion &A = e.occlusion;
    const bool point = L.kind == RTDD_LIGHT_POINT;
    if (occlusion_cannot_show(A)) return launch_relight_shadow(ctx, e);
    if (shadow_cannot_show(L, S)) return launch_ambient_occlusion(ctx, e);
    if (A.radius < 0 || A.radius > kAoMaxRadius) return fail(ctx, RTDD_ERR_INVALID, "lighting: radius outside [0, 64]");
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, L.anchorX, L.anchorY) : nullptr;
    ao_radius_class(A.radius, [&](auto c) { launch_class<decltype(c)::RMAX, decltype(c)::NW>(ctx, e, T, anchor_px); });
    RTDD_LAUNCH_CHECK(ctx, "k_lighting");
    return RTDD_OK;
}

}  // namespace rtdd
