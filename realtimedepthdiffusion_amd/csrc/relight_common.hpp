// relight_common.hpp -- the shading arithmetic that relight.hip (k_relight), relight_shadow.hip (k_relight_shadow),
// ambient_occlusion.hip (k_ambient_occlusion) and lighting.hip (k_lighting) share: the depth clamp, the shade of one pixel, the byte of one channel.  The header's lines (include/rtdd.h rtdd_simulate_relight), operation by
// operation; both translation units are compiled with -ffp-contract=off and hold no fmaf.
// Included inside no namespace; everything here is in namespace rtdd.
#pragma once

#include <cmath>

#include "rtdd_internal.hpp"

namespace rtdd {

typedef Effect::Light Light;

__device__ __forceinline__ float clamp_depth(float d) { return fminf(fmaxf(d, 0.0f), 255.0f); }     // a NaN depth is 0 (stereo's clamp)

// The shade of pixel (x, y): dc its clamped depth, dl / dr / du / dd its left / right / upper / lower neighbours' (replicated border).
// Lz: the point light's height in scene units (wave-uniform).
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

// (uchar) fminf(o * (ambient + (k_c * shade)), 255): the gain is finite and >= 0, so the truncation is defined
__device__ __forceinline__ uint32_t relight_u8(const Light &L, int c, float shade, uint32_t o) {
    return (uint32_t)(int)fminf((float)o * (L.ambient + (L.k[c] * shade)), 255.0f);
}

// the same byte with the ambient term the caller occluded, amb = ambient * ao (rtdd_simulate_ambient_occlusion under a light)
__device__ __forceinline__ uint32_t relight_u8_ambient(const Light &L, int c, float amb, float shade, uint32_t o) {
    return (uint32_t)(int)fminf((float)o * (amb + (L.k[c] * shade)), 255.0f);
}

// What ambient_occlusion.hip (k_ambient_occlusion) and lighting.hip (k_lighting) share of the occlusion: the tile, and the tables.
constexpr int kAoW = 64, kAoH = 16;                                 // the tile: a wave's 64 lanes wide
constexpr int kAoMaxRadius = 64;
// inv_j[k] at [k - 1]: the axis directions' and the diagonals'.  They depend on k alone, so they are built once on the host and
// travel to every launch by value, a replay's included.
struct AoTables { float axis[kAoMaxRadius], diag[kAoMaxRadius]; };

inline AoTables ao_tables() {
    AoTables t;
    for (int k = 1; k <= kAoMaxRadius; k++) {
        t.axis[k - 1] = (float)(1.0 / (double)k);
        t.diag[k - 1] = (float)(1.0 / ((double)k * std::sqrt(2.0)));
    }
    return t;
}

}  // namespace rtdd
