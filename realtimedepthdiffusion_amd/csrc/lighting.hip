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

typedef Effect::Shadow Shadow;
typedef Effect::Occlusion Occlusion;

constexpr int kLtGroup = 4;          // steps of the march per group of loads (k_relight_shadow's)

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

    // staging: rows y0 - r .. y0 + 15 + r, columns x0 - r .. x0 + 63 + r; a wave a row at a time, its lanes consecutive words
    const int rw = kAoW + 2 * r, rh = kAoH + 2 * r;
    for (int ry = wave; ry < rh; ry += NW) {
        const int gy = y0 - r + ry;
        const bool row_inside = (unsigned)gy < (unsigned)rows;       // (wave-uniform)
        const float *srow = (const float *)((const char *)depth + (size_t)(row_inside ? gy : 0) * dp);
        float *hrow = Hs + (RMAX - r + ry) * P + (RMAX - r);
        for (int rx = lane; rx < rw; rx += 64) {
            const int gx = x0 - r + rx;
            float h = -INFINITY;
            if (row_inside && (unsigned)gx < (unsigned)cols) h = A.relief * (255.0f - clamp_depth(srow[gx]));
            hrow[rx] = h;
        }
    }
    __syncthreads();                                                 // the one barrier: every wave reaches it

    constexpr int ux[8] = {1, 1, 0, -1, -1, -1, 0, 1}, uy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    float Lz = 0.0f;
    if (POINT) {
        const float dA = anchor_px ? clamp_depth(*anchor_px) : L.anchorDepth;
        Lz = (L.relief * (255.0f - dA)) + L.z;
    }
    const bool soft = S.softness > 0.0f;                             // (wave-uniform)
    const float hmax = L.relief * 255.0f;
    for (int ty = wave; ty < kAoH; ty += NW) {
        const int x = x0 + lane, y = y0 + ty;
        const float *own = Hs + (RMAX + ty) * P + RMAX + lane;
        const float h = *own;                                        // H(x, y); minus infinity beyond the image (such a lane stores nothing)

        // the horizons: k_ambient_occlusion's march over the staged heights
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

        // k_relight's shade from the map itself (replicated border)
        const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
        const float *urow = (const float *)((const char *)depth + (size_t)max(y - 1, 0) * dp);
        const float *lrow = (const float *)((const char *)depth + (size_t)min(y + 1, rows - 1) * dp);
        const float shade = relight_shade<POINT>(L, Lz, clamp_depth(drow[x]), clamp_depth(drow[max(x - 1, 0)]), clamp_depth(drow[min(x + 1, cols - 1)]),
                                                 clamp_depth(urow[x]), clamp_depth(lrow[x]), x, y);

        // k_relight_shadow's march.  Its direction: the record's (a directional light), or this pixel's own towards the point light
        float sx = S.sx, sy = S.sy, rise = S.rise;
        int n = S.maxSteps;
        if (POINT) {
            const float vx = L.x - (float)x, vy = L.y - (float)y, vz = Lz - h;
            const float m = fmaxf(fabsf(vx), fabsf(vy));
            if (m < 1.0f) { n = 0; sx = sy = rise = 0.0f; }             // the light stands over this pixel: lit
            else { sx = vx / m; sy = vy / m; rise = vz / m; n = min(n, (int)m); }
        }
        // the steps that stay inside the IMAGE (not the staged region): the largest k <= n whose (px, py) is inside; monotonic in k,
        // so the bound is exact and the march below tests none
        const auto inside = [&](int k) {
            const float kf = (float)k;
            return (unsigned)(x + (int)rintf(kf * sx)) < (unsigned)cols && (unsigned)(y + (int)rintf(kf * sy)) < (unsigned)rows;
        };
        if (n > 0 && !inside(n)) {
            int lo = 0;                                                  // inside(lo), !inside(n)
            while (n - lo > 1) {
                const int mid = (lo + n) >> 1;
                if (inside(mid)) lo = mid; else n = mid;
            }
            n = lo;
        }
        // a group that reaches past n repeats step n, which a maximum does not see
        const float h0 = h + S.bias;
        const char *ownd = (const char *)(drow + x);
        float q = 0.0f;
        for (int k0 = 1; k0 <= n; k0 += kLtGroup) {
            float dv[kLtGroup];
#pragma unroll
            for (int j = 0; j < kLtGroup; j++) {
                const float kf = (float)min(k0 + j, n);
                const int dx = (int)rintf(kf * sx), dy = (int)rintf(kf * sy);
                dv[j] = *(const float *)(ownd + ((ptrdiff_t)dy * (ptrdiff_t)dp + (ptrdiff_t)dx * 4));
            }
            float ray = 0.0f;
#pragma unroll
            for (int j = 0; j < kLtGroup; j++) {
                const float kf = (float)min(k0 + j, n);
                ray = h0 + (kf * rise);
                const float occ = (L.relief * (255.0f - clamp_depth(dv[j]))) - ray;
                if (occ > 0.0f) q = soft ? fmaxf(q, fminf(occ / (kf * S.softness), 1.0f)) : 1.0f;
            }
            // over: a full shadow, or the ray has risen above every height (rise >= 0: it stays there)
            if (q == 1.0f || (rise >= 0.0f && ray > hmax)) break;
        }
        const float lit = shade * (1.0f - (S.strength * q));
        const float amb = L.ambient * ao;
        const uint8_t *o = orig + (size_t)y * op + 3 * (size_t)x;
        uint8_t *a = art + (size_t)y * ap + 3 * (size_t)x;
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8_ambient(L, c, amb, lit, o[c]);
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
    if (A.radius == 0 || A.strength == 0.0f || A.relief == 0.0f) return launch_relight_shadow(ctx, e);
    if (S.maxSteps == 0 || S.strength == 0.0f || (!point && S.sx == 0.0f && S.sy == 0.0f)) return launch_ambient_occlusion(ctx, e);
    if (A.radius < 0 || A.radius > kAoMaxRadius) return fail(ctx, RTDD_ERR_INVALID, "lighting: radius outside [0, 64]");
    const float *anchor_px = point ? pixel_ptr(e.depth, e.depthPitch, L.anchorX, L.anchorY) : nullptr;
    if (A.radius <= 8) launch_class<8, 4>(ctx, e, T, anchor_px);
    else if (A.radius <= 16) launch_class<16, 4>(ctx, e, T, anchor_px);
    else if (A.radius <= 32) launch_class<32, 8>(ctx, e, T, anchor_px);
    else launch_class<64, 16>(ctx, e, T, anchor_px);
    RTDD_LAUNCH_CHECK(ctx, "k_lighting");
    return RTDD_OK;
}

}  // namespace rtdd
