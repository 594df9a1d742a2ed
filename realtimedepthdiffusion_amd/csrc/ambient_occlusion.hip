// ambient_occlusion.hip -- ambient occlusion from the depth map (rtdd_simulate_ambient_occlusion, include/rtdd.h): from every pixel the
// horizon of the height field H = relief * (255 - d') along 4 or 8 compass directions over `radius` pixels; alone (the original
// darkened, or the occlusion as a gray map) or as the ambient term of k_relight's shading.  One launch.
//
// A bounded gather from LDS.  A workgroup owns a tile of 64 x 16 pixels and stages H ONCE for the tile and a halo of `radius` pixels on
// every side: clamped, subtracted and multiplied once per height, not once per sample, and a position outside the image is written as
// minus infinity, which no maximum ever takes -- so the march holds no bounds test, no clamp and no address product.  One barrier
// orders the staging before the marches; nothing returns in front of it.  Then a wave takes a row of the tile, its lanes 64 consecutive
// x: at step k of any of the eight directions the wave reads 64 consecutive LDS words, free of bank conflicts whatever the pitch.  The
// LDS pitch is a constant of the instantiation, so the position of step k in direction j is the pixel's own word plus the constant
// k * (uy * pitch + ux).  Every staged height is read by up to 8 * radius marches.
//
// The tile is the same for every radius, the LDS array and the workgroup are not: the array holds the halo of the largest radius of
// its class -- 8, 16, 32 or 64: 10, 18, 40 and 108 KiB of the CU's 160 -- and a class whose array leaves room for several workgroups
// per CU runs small ones (4 or 8 waves, a wave walks 4 or 2 rows), while the 108 KiB of radius 33 .. 64 admit one workgroup per CU,
// which therefore brings all 16 waves the tile has rows for.  Within a class only the halo the radius needs is staged.
//
// The arithmetic is the header's, operation by operation: compiled like relight.hip with -ffp-contract=off, no fmaf, the correctly
// rounded `/` and sqrtf, denormals kept -- the bytes are those of tests/ao_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.  The
// header's early exit (no later step can win) is not taken: the lanes of a wave would have to agree on it.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"
#include "relight_common.hpp"

namespace rtdd {

enum : int { kAoOutShade = 0, kAoOutMap = 1, kAoOutDirectional = 2, kAoOutPoint = 3 };     // the first two are rtdd_ao_mode's

// RMAX: the largest radius the LDS array has a halo for; NW: waves per workgroup; DIRS: 4 or 8; OUT: what is written.
template <int RMAX, int NW, int DIRS, int OUT>
__global__ __launch_bounds__(64 * NW) void k_ambient_occlusion(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                               uint8_t *__restrict__ art, size_t ap, int rows, int cols, Occlusion A, Light L,
                                                               AoTables T, const float *__restrict__ anchor_px) {
    constexpr int P = kAoW + 2 * RMAX;                               // words per LDS row
    __shared__ float Hs[(kAoH + 2 * RMAX) * P];                      // Hs[(RMAX + ty) * P + RMAX + tx] = H(x0 + tx, y0 + ty)
    static_assert(sizeof(Hs) <= 160 * 1024 && NW <= kAoH && kAoH % NW == 0, "the tile with its halo fits a CU's LDS; every wave walks the same number of rows");
    const int r = A.radius;                                          // <= RMAX (launch_ambient_occlusion)
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * kAoW, y0 = blockIdx.y * kAoH;
    ao_stage<RMAX, NW>(Hs, depth, dp, rows, cols, x0, y0, r, A.relief, wave, lane);
    __syncthreads();                                                 // the one barrier: every wave reaches it

    const float Lz = OUT == kAoOutPoint ? point_light_height(L, anchor_px) : 0.0f;
    for (int ty = wave; ty < kAoH; ty += NW) {
        const int x = x0 + lane, y = y0 + ty;
        const float *own = Hs + (RMAX + ty) * P + RMAX + lane;
        const float ao = ao_factor<RMAX, DIRS>(own, *own, A, T, r);  // H(x, y) is minus infinity beyond the image (such a lane stores nothing)
        if (x >= cols || y >= rows) continue;                        // (behind the barrier; no cross-lane operation below)
        uint8_t *a = art + (size_t)y * ap + 3 * (size_t)x;
        if (OUT == kAoOutMap) {
            a[0] = a[1] = a[2] = (uint8_t)(int)(255.0f * ao);
            continue;
        }
        const uint8_t *o = orig + (size_t)y * op + 3 * (size_t)x;
        if (OUT == kAoOutShade) {
#pragma unroll
            for (int c = 0; c < 3; c++) a[c] = (uint8_t)(int)((float)o[c] * ao);
            continue;
        }
        // under a light: k_relight's shade from the map itself, the ambient term occluded
        float dc;
        const float shade = shade_at<OUT == kAoOutPoint>(L, Lz, depth, dp, rows, cols, x, y, dc);
        const float amb = L.ambient * ao;
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8(L, c, amb, shade, o[c]);
    }
}

template <int RMAX, int NW>
static void launch_class(rtdd_ctx *ctx, const Effect &e, const Occlusion &A, const AoTables &T, int out, const float *anchor_px) {
    const dim3 g((e.cols + kAoW - 1) / kAoW, (e.rows + kAoH - 1) / kAoH);
#define RTDD_AO_LAUNCH(D, O) hipLaunchKernelGGL((k_ambient_occlusion<RMAX, NW, D, O>), g, dim3(64 * NW), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols, A, e.light, T, anchor_px)
#define RTDD_AO_DIRS(O) do { if (A.directions == 4) RTDD_AO_LAUNCH(4, O); else RTDD_AO_LAUNCH(8, O); } while (0)
    switch (out) {
        case kAoOutShade: RTDD_AO_DIRS(kAoOutShade); break;
        case kAoOutMap: RTDD_AO_DIRS(kAoOutMap); break;
        case kAoOutDirectional: RTDD_AO_DIRS(kAoOutDirectional); break;
        default: RTDD_AO_DIRS(kAoOutPoint); break;
    }
#undef RTDD_AO_DIRS
#undef RTDD_AO_LAUNCH
}

// rtdd_simulate_ambient_occlusion (arguments checked, the light prepared by effects_api.cpp): one launch.  The class is the smallest
// whose halo holds the radius; where no horizon can count -- no strength, a flat surface -- the march is left out (ao == 1 either way).
int launch_ambient_occlusion(rtdd_ctx *ctx, const Effect &e) {
    static const AoTables T = ao_tables();
    Occlusion A = e.occlusion;
    if (occlusion_cannot_show(A)) A.radius = 0;
    if (A.radius < 0 || A.radius > kAoMaxRadius) return fail(ctx, RTDD_ERR_INVALID, "ambient occlusion: radius outside [0, 64]");
    const bool point = A.lit && e.light.kind == RTDD_LIGHT_POINT;
    const int out = A.lit ? (point ? kAoOutPoint : kAoOutDirectional) : (A.mode == RTDD_AO_MAP ? kAoOutMap : kAoOutShade);
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, e.light.anchorX, e.light.anchorY) : nullptr;
    ao_radius_class(A.radius, [&](auto c) { launch_class<decltype(c)::RMAX, decltype(c)::NW>(ctx, e, A, T, out, anchor_px); });
    RTDD_LAUNCH_CHECK(ctx, "k_ambient_occlusion");
    return RTDD_OK;
}

}  // namespace rtdd
