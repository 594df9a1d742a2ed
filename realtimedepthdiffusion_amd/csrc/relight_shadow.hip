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

typedef Effect::Shadow Shadow;

constexpr int kShGroup = 4;          // steps per group of loads

template <bool POINT, bool SOFT>
__global__ __launch_bounds__(256) void k_relight_shadow(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                        uint8_t *__restrict__ art, size_t ap, int rows, int cols, Light L, Shadow S,
                                                        const float *__restrict__ anchor_px) {
    const int y = blockIdx.y * 4 + wave_id();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (y >= rows || x >= cols) return;                              // (no cross-lane operation below)
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const float *urow = (const float *)((const char *)depth + (size_t)max(y - 1, 0) * dp);
    const float *lrow = (const float *)((const char *)depth + (size_t)min(y + 1, rows - 1) * dp);
    float Lz = 0.0f;
    if (POINT) {
        const float dA = anchor_px ? clamp_depth(*anchor_px) : L.anchorDepth;
        Lz = (L.relief * (255.0f - dA)) + L.z;
    }
    const float dc = clamp_depth(drow[x]);
    const float shade = relight_shade<POINT>(L, Lz, dc, clamp_depth(drow[max(x - 1, 0)]), clamp_depth(drow[min(x + 1, cols - 1)]),
                                             clamp_depth(urow[x]), clamp_depth(lrow[x]), x, y);
    const float h = L.relief * (255.0f - dc);                        // H(x, y)

    // the direction of the march: the record's (a directional light), or this pixel's own towards the point light
    float sx = S.sx, sy = S.sy, rise = S.rise;
    int n = S.maxSteps;
    if (POINT) {
        const float vx = L.x - (float)x, vy = L.y - (float)y, vz = Lz - h;
        const float m = fmaxf(fabsf(vx), fabsf(vy));
        if (m < 1.0f) { n = 0; sx = sy = rise = 0.0f; }             // the light stands over this pixel: lit
        else { sx = vx / m; sy = vy / m; rise = vz / m; n = min(n, (int)m); }
    }

    // The steps that stay inside the image: the largest k <= n whose (px, py) is inside.  fl(kf * s) and rintf are monotonic in k and
    // keep the sign of s, so a position that has left the image never returns -- "the first k outside ends the march" is "k <= n".
    // Most pixels' last step is inside (one test); the others bisect with the march's own f32 expressions, so the bound is exact.
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

    // The march: no bounds test, no branch round a load.  A group that reaches past n repeats step n, which a maximum does not see.
    const float h0 = h + S.bias, hmax = L.relief * 255.0f;
    const char *own = (const char *)(drow + x);
    float q = 0.0f;
    for (int k0 = 1; k0 <= n; k0 += kShGroup) {
        float dv[kShGroup];
#pragma unroll
        for (int j = 0; j < kShGroup; j++) {
            const float kf = (float)min(k0 + j, n);
            const int dx = (int)rintf(kf * sx), dy = (int)rintf(kf * sy);
            dv[j] = *(const float *)(own + ((ptrdiff_t)dy * (ptrdiff_t)dp + (ptrdiff_t)dx * 4));
        }
        float ray = 0.0f;
#pragma unroll
        for (int j = 0; j < kShGroup; j++) {
            const float kf = (float)min(k0 + j, n);
            ray = h0 + (kf * rise);
            const float occ = (L.relief * (255.0f - clamp_depth(dv[j]))) - ray;
            if (occ > 0.0f) q = SOFT ? fmaxf(q, fminf(occ / (kf * S.softness), 1.0f)) : 1.0f;
        }
        // over: a full shadow, or the ray has risen above every height (rise >= 0: it stays there)
        if (q == 1.0f || (rise >= 0.0f && ray > hmax)) break;
    }
    const float lit = shade * (1.0f - (S.strength * q));
    const uint8_t *o = orig + (size_t)y * op + 3 * (size_t)x;
    uint8_t *a = art + (size_t)y * ap + 3 * (size_t)x;
#pragma unroll
    for (int c = 0; c < 3; c++) a[c] = (uint8_t)relight_u8(L, c, lit, o[c]);
}

// rtdd_simulate_relight_shadowed (arguments checked, the light and the direction prepared by effects_api.cpp): one launch.  Where no pixel can
// be shadowed -- no steps, no strength, a directional light straight above (m == 0: sx == sy == 0) -- the launch is k_relight's own.
int launch_relight_shadow(rtdd_ctx *ctx, const Effect &e) {
    const Light &L = e.light;
    const Shadow &S = e.shadow;
    const bool point = L.kind == RTDD_LIGHT_POINT;
    if (S.maxSteps == 0 || S.strength == 0.0f || (!point && S.sx == 0.0f && S.sy == 0.0f)) return launch_relight(ctx, e);
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
