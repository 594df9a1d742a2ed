// relight_common.hpp -- the lighting model's steps, each stated once, for relight.hip (k_relight), relight_shadow.hip (k_relight_shadow),
// ambient_occlusion.hip (k_ambient_occlusion) and lighting.hip (k_lighting).  Device: the point light's height, the shade of one pixel
// (from its depths, and from the map itself), the march towards the light, the staging of the heights and the horizons over them, the
// byte of one channel.  Host: the occlusion's tables and radius classes, and the two rules by which a term cannot show.  Why each kernel
// has its shape is told in the kernel's own file.
// The arithmetic is the header's (include/rtdd.h rtdd_simulate_relight, _relight_shadowed, _ambient_occlusion), operation by operation;
// every translation unit that includes this is compiled with -ffp-contract=off and holds no fmaf.
// Included inside no namespace; everything here is in namespace rtdd.
#pragma once

#include <cmath>

#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

typedef Effect::Light Light;
typedef Effect::Shadow Shadow;
typedef Effect::Occlusion Occlusion;

// Lz: the point light's height in scene units.  The anchor is one uniform load per wave (the pixel form reads the map when the kernel
// runs, as refocus's focus).
__device__ __forceinline__ float point_light_height(const Light &L, const float *__restrict__ anchor_px) {
    const float dA = anchor_px ? clamp_depth(*anchor_px) : L.anchorDepth;
    return (L.relief * (255.0f - dA)) + L.z;
}

// The shade of pixel (x, y): dc its clamped depth, dl / dr / du / dd its left / right / upper / lower neighbours' (replicated border).
// Lz: the point light's height (wave-uniform).
template <bool POINT>
__device__ __forceinline__ float relight_shade(const Light &L, float Lz, float dc, float dl, float dr, float du, float dd, int x, int y) {
    const float gx = dr - dl, gy = dd - du;
    const float nx = L.relief * gx, ny = L.relief * gy;
    const float nn = ((nx * nx) + (ny * ny)) + 4.0f;
    if (!POINT) {
        const float dot = ((nx * L.x) + (ny * L.y)) + (2.0f * L.z);
        return fmaxf(dot, 0.0f) / sqrtf(nn);
    }
    const float vx = L.x - (float)x, vy = L.y - (float)y, vz = Lz - (L.relief * (255.0f - dc));
    const float vv = ((vx * vx) + (vy * vy)) + (vz * vz);
    const float dot = ((nx * vx) + (ny * vy)) + (2.0f * vz);
    const float s = (fmaxf(dot, 0.0f) / sqrtf(nn * vv)) / (1.0f + (vv * L.invR2));
    return vv == 0.0f ? 0.0f : s;
}

// The same shade with every depth from the map itself, replicated border; dc: the pixel's own clamped depth, for the caller.
// shade_in_rows: drow the pixel's row of the map, urow / lrow the rows above and below it as shade_at takes them.
template <bool POINT>
__device__ __forceinline__ float shade_in_rows(const Light &L, float Lz, const float *__restrict__ drow, const float *__restrict__ urow,
                                               const float *__restrict__ lrow, int cols, int x, int y, float &dc) {
    dc = clamp_depth(drow[x]);
    return relight_shade<POINT>(L, Lz, dc, clamp_depth(drow[max(x - 1, 0)]), clamp_depth(drow[min(x + 1, cols - 1)]), clamp_depth(urow[x]),
                                clamp_depth(lrow[x]), x, y);
}
template <bool POINT>
__device__ __forceinline__ float shade_at(const Light &L, float Lz, const float *__restrict__ depth, size_t dp, int rows, int cols, int x, int y,
                                          float &dc) {
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const float *urow = (const float *)((const char *)depth + (size_t)max(y - 1, 0) * dp);
    const float *lrow = (const float *)((const char *)depth + (size_t)min(y + 1, rows - 1) * dp);
    return shade_in_rows<POINT>(L, Lz, drow, urow, lrow, cols, x, y, dc);
}

// (uchar) fminf(o * (amb + (k_c * shade)), 255): the gain is finite and >= 0, so the truncation is defined.  amb: L.ambient, or the
// ambient term the caller occluded, ambient * ao.
__device__ __forceinline__ uint32_t relight_u8(const Light &L, int c, float amb, float shade, uint32_t o) {
    return (uint32_t)(int)fminf((float)o * (amb + (L.k[c] * shade)), 255.0f);
}

// ---- the march towards the light (include/rtdd.h rtdd_simulate_relight_shadowed) ----
constexpr int kShGroup = 4;          // steps per group of loads

// q of pixel (x, y) of height h: drow its depth row, Lz the point light's height.  SOFT: 1 the penumbra's division is taken, 0 it is
// not (k_relight_shadow's two instantiations), kSoftByRecord it is where the record's softness > 0 -- wave-uniform, a scalar branch
// (k_lighting, whose instantiations it would double).
constexpr int kSoftByRecord = -1;
template <bool POINT, int SOFT>
__device__ __forceinline__ float shadow_march(const Light &L, const Shadow &S, float Lz, float h, const float *__restrict__ drow, size_t dp, int x,
                                              int y, int rows, int cols) {
    const bool soft = SOFT == kSoftByRecord ? S.softness > 0.0f : SOFT != 0;
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
            if (occ > 0.0f) q = soft ? fmaxf(q, fminf(occ / (kf * S.softness), 1.0f)) : 1.0f;
        }
        // over: a full shadow, or the ray has risen above every height (rise >= 0: it stays there)
        if (q == 1.0f || (rise >= 0.0f && ray > hmax)) break;
    }
    return q;
}

// ---- the occlusion (include/rtdd.h rtdd_simulate_ambient_occlusion) ----
constexpr int kAoW = 64, kAoH = 16;                                 // the tile: a wave's 64 lanes wide
constexpr int kAoMaxRadius = 64;
// inv_j[k] at [k - 1]: the axis directions' and the diagonals'.  They depend on k alone, so they are built once on the host and
// travel to every launch by value, a replay's included.
struct AoTables { float axis[kAoMaxRadius], diag[kAoMaxRadius]; };

// Staging.  Hs[(RMAX + ty) * P + RMAX + tx] = H(x0 + tx, y0 + ty) = relief * (255 - d'), P = kAoW + 2 * RMAX words per LDS row, minus
// infinity outside the image: rows y0 - r .. y0 + 15 + r, columns x0 - r .. x0 + 63 + r; a wave (of NW) a row at a time, its lanes
// consecutive words.  The barrier behind it is the caller's.
template <int RMAX, int NW>
__device__ __forceinline__ void ao_stage(float *__restrict__ Hs, const float *__restrict__ depth, size_t dp, int rows, int cols, int x0, int y0, int r,
                                         float relief, int wave, int lane) {
    constexpr int P = kAoW + 2 * RMAX;
    const int rw = kAoW + 2 * r, rh = kAoH + 2 * r;
    for (int ry = wave; ry < rh; ry += NW) {
        const int gy = y0 - r + ry;
        const bool row_inside = (unsigned)gy < (unsigned)rows;       // (wave-uniform)
        const float *drow = (const float *)((const char *)depth + (size_t)(row_inside ? gy : 0) * dp);
        float *hrow = Hs + (RMAX - r + ry) * P + (RMAX - r);
        for (int rx = lane; rx < rw; rx += 64) {
            const int gx = x0 - r + rx;
            float h = -INFINITY;
            if (row_inside && (unsigned)gx < (unsigned)cols) h = relief * (255.0f - clamp_depth(drow[gx]));
            hrow[rx] = h;
        }
    }
}

// ao of the pixel whose staged height is h = *own: the horizons of DIRS directions over r steps.  The position of step k in direction j
// is the pixel's own word plus the constant k * (uy * P + ux).
template <int RMAX, int DIRS>
__device__ __forceinline__ float ao_factor(const float *__restrict__ own, float h, const Occlusion &A, const AoTables &T, int r) {
    constexpr int P = kAoW + 2 * RMAX;
    constexpr int ux[8] = {1, 1, 0, -1, -1, -1, 0, 1}, uy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    float tmax[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int k = 1; k <= r; k++) {
        const float ia = T.axis[k - 1], id = T.diag[k - 1];          // (wave-uniform)
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
    return 1.0f - (A.strength * mean);
}

// ---- host ----
inline AoTables ao_tables() {
    AoTables t;
    for (int k = 1; k <= kAoMaxRadius; k++) {
        t.axis[k - 1] = (float)(1.0 / (double)k);
        t.diag[k - 1] = (float)(1.0 / ((double)k * std::sqrt(2.0)));
    }
    return t;
}

// The radius classes: the LDS array holds the halo of the largest radius of its class (RMAX), and a class whose array leaves room for
// several workgroups per CU runs small ones (NW waves; ambient_occlusion.hip tells why).  f(AoClass<RMAX, NW>()) for the smallest class
// whose halo holds `radius` (<= kAoMaxRadius).
template <int RMAX_, int NW_> struct AoClass { static constexpr int RMAX = RMAX_, NW = NW_; };
template <class F>
inline void ao_radius_class(int radius, F &&f) {
    if (radius <= 8) f(AoClass<8, 4>());
    else if (radius <= 16) f(AoClass<16, 4>());
    else if (radius <= 32) f(AoClass<32, 8>());
    else f(AoClass<64, 16>());
}

// no pixel can be shadowed: no steps, no strength, a directional light straight above (m == 0: sx == sy == 0) -- vis == 1
inline bool shadow_cannot_show(const Light &L, const Shadow &S) {
    return S.maxSteps == 0 || S.strength == 0.0f || (L.kind != RTDD_LIGHT_POINT && S.sx == 0.0f && S.sy == 0.0f);
}
// no horizon can count: no radius, no strength, a flat surface -- ao == 1
inline bool occlusion_cannot_show(const Occlusion &A) { return A.radius == 0 || A.strength == 0.0f || A.relief == 0.0f; }

}  // namespace rtdd
