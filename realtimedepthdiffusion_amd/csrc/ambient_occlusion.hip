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

typedef Effect::Occlusion Occlusion;

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

    // staging: rows y0 - r .. y0 + 15 + r, columns x0 - r .. x0 + 63 + r; a wave a row at a time, its lanes consecutive words
    const int rw = kAoW + 2 * r, rh = kAoH + 2 * r;
    for (int ry = wave; ry < rh; ry += NW) {
        const int gy = y0 - r + ry;
        const bool row_inside = (unsigned)gy < (unsigned)rows;       // (wave-uniform)
        const float *drow = (const float *)((const char *)depth + (size_t)(row_inside ? gy : 0) * dp);
        float *hrow = Hs + (RMAX - r + ry) * P + (RMAX - r);
        for (int rx = lane; rx < rw; rx += 64) {
            const int gx = x0 - r + rx;
            float h = -INFINITY;
            if (row_inside && (unsigned)gx < (unsigned)cols) h = A.relief * (255.0f - clamp_depth(drow[gx]));
            hrow[rx] = h;
        }
    }
    __syncthreads();                                                 // the one barrier: every wave reaches it

    constexpr int ux[8] = {1, 1, 0, -1, -1, -1, 0, 1}, uy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    float Lz = 0.0f;
    if (OUT == kAoOutPoint) {
        const float dA = anchor_px ? clamp_depth(*anchor_px) : L.anchorDepth;
        Lz = (L.relief * (255.0f - dA)) + L.z;
    }
    for (int ty = wave; ty < kAoH; ty += NW) {
        const int x = x0 + lane, y = y0 + ty;
        const float *own = Hs + (RMAX + ty) * P + RMAX + lane;
        const float h = *own;                                        // H(x, y); minus infinity beyond the image (such a lane stores nothing)
        float tmax[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int k = 1; k <= r; k++) {
            const float ia = T.axis[k - 1], id = T.diag[k - 1];      // (wave-uniform)
#pragma unroll
            for (int j = 0; j < 8; j += 8 / DIRS) {
                const float rise = (own[k * (uy[j] * P + ux[j])] - h) - A.bias;
                tmax[j] = fmaxf(tmax[j], rise * ((j & 1) ? id : ia));
            }
        }
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j += 8 / DIRS) {
            const float occ = tmax[j] / sqrtf(1.0f + (tmax[j] * tmax[j]));
            s = j == 0 ? occ : s + occ;
        }
        const float mean = s * (1.0f / (float)DIRS);
        const float ao = 1.0f - (A.strength * mean);
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
        // under a light: k_relight's shade from the map itself (replicated border), the ambient term occluded
        const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
        const float *urow = (const float *)((const char *)depth + (size_t)max(y - 1, 0) * dp);
        const float *lrow = (const float *)((const char *)depth + (size_t)min(y + 1, rows - 1) * dp);
        const float shade = relight_shade<OUT == kAoOutPoint>(L, Lz, clamp_depth(drow[x]), clamp_depth(drow[max(x - 1, 0)]),
                                                              clamp_depth(drow[min(x + 1, cols - 1)]), clamp_depth(urow[x]), clamp_depth(lrow[x]), x, y);
        const float amb = L.ambient * ao;
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8_ambient(L, c, amb, shade, o[c]);
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
    if (A.strength == 0.0f || A.relief == 0.0f) A.radius = 0;
    if (A.radius < 0 || A.radius > kAoMaxRadius) return fail(ctx, RTDD_ERR_INVALID, "ambient occlusion: radius outside [0, 64]");
    const bool point = A.lit && e.light.kind == RTDD_LIGHT_POINT;
    const int out = A.lit ? (point ? kAoOutPoint : kAoOutDirectional) : (A.mode == RTDD_AO_MAP ? kAoOutMap : kAoOutShade);
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, e.light.anchorX, e.light.anchorY) : nullptr;
    if (A.radius <= 8) launch_class<8, 4>(ctx, e, A, T, out, anchor_px);
    else if (A.radius <= 16) launch_class<16, 4>(ctx, e, A, T, out, anchor_px);
    else if (A.radius <= 32) launch_class<32, 8>(ctx, e, A, T, out, anchor_px);
    else launch_class<64, 16>(ctx, e, A, T, out, anchor_px);
    RTDD_LAUNCH_CHECK(ctx, "k_ambient_occlusion");
    return RTDD_OK;
}

}  // namespace rtdd
