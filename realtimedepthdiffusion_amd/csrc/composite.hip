// composite.hip -- a sprite inserted into the scene at a depth (rtdd_composite_layer, include/rtdd.h; DESIGN.md section 4 "Composite"):
// the scene's depth map hides what lies behind nearer things, and the composite's own depth map is written beside the image.
//
// A stream like haze_ex and relight (3 B + 4 B read, 3 B + 4 B written per pixel outside the sprite): a lane takes FOUR pixels of a
// row -- the image as three dwords in and out, the depth as one float4 in and out -- a wave 256 pixels of one row, a workgroup four
// rows.  Rows that are not aligned for that take one pixel per lane with the same arithmetic.  The host passes the sprite's clipped
// footprint: a lane whose pixels miss it copies, and so does every wave of a workgroup whose tile misses it (the branch is wave-uniform
// wherever the footprint's edges allow; a row is one wave).  Inside the footprint the sprite's texels are plain global loads.  No LDS,
// no atomics; every pixel of both outputs is stored exactly once.
//
// The arithmetic is the header's, operation by operation.  Integers are exact: the two floor divisions of step 1 and `div A` of step 2
// are 32-bit unsigned divisions whose operands are proven to fit (below), `div E` divides by a constant.  The floats of steps 3 and 4
// are single operations: this translation unit is compiled with -ffp-contract=off and holds no fmaf, `/` is the correctly rounded one
// (-fhip-fp32-correctly-rounded-divide-sqrt), denormals are kept -- the bytes and the depth's bits are those of tests/composite_ref.py
// and do not depend on RTDD_OPT_FP_CONTRACT.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

typedef Effect::Composite Composite;

constexpr uint32_t kLayerE = 255u * 255u * 256u;                     // E: the largest a * opacity * v

// Step 1 along one axis: q = U + 128 = floor(((2 (p - origin) + 1) * 32768) / scale) for p >= origin.  The footprint starts at the
// sprite's corner, so p - origin >= 0; p < 46341 (rows^2 + cols^2 < 2^31) and origin >= -16384 give 2 (p - origin) + 1 < 125451, and
// 125451 * 32768 < 2^32: the numerator fits 32 bits unsigned, where the division is exact.  q < 2^32 / 16.
__device__ __forceinline__ uint32_t layer_coord(int p, int origin, uint32_t scale) {
    return ((2u * (uint32_t)(p - origin) + 1u) * 32768u) / scale;
}

// texel (tx, ty) as b | g << 8 | r << 16 | a << 24; `aligned`: every row of the sprite starts at a multiple of 4 bytes (uniform)
__device__ __forceinline__ uint32_t texel(const uint8_t *__restrict__ srow, int tx, bool aligned) {
    const uint8_t *q = srow + 4 * (size_t)tx;
    if (aligned) return *(const uint32_t *)q;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}

// What a row of the image needs of the layer, the same for every pixel of the row (a wave is one row: scalar work).
struct LayerRow {
    bool covered;                               // step 1 in y
    const uint8_t *s0, *s1;                     // the sprite rows of the taps (NEAREST: s0 only)
    uint32_t fv;                                // BILINEAR
    long long ny;                               // (py - y0)(y1 - y0)
};

template <int FILTER>
__device__ __forceinline__ LayerRow layer_row(const Composite &k, int py) {
    const rtdd_layer &L = k.layer;
    LayerRow r;
    r.ny = (long long)(py - L.y0) * (L.y1 - L.y0);
    r.s0 = r.s1 = k.sprite; r.fv = 0;
    r.covered = py >= k.fy0 && py < k.fy1;
    if (!r.covered) return r;
    const uint32_t q = layer_coord(py, L.y, (uint32_t)L.scale);
    r.covered = q < 256u * (uint32_t)L.rows;
    if (!r.covered) return r;
    if (FILTER == RTDD_LAYER_NEAREST) {
        r.s0 = k.sprite + (size_t)(q >> 8) * k.spritePitch;
    } else {
        const int V = (int)q - 128, iv = V >> 8;                    // (an arithmetic shift: the floor)
        r.fv = (uint32_t)(V & 255);
        r.s0 = k.sprite + (size_t)min(max(iv, 0), L.rows - 1) * k.spritePitch;
        r.s1 = k.sprite + (size_t)min(max(iv + 1, 0), L.rows - 1) * k.spritePitch;
    }
    return r;
}

// One pixel of a covered row: o its original as b | g << 8 | r << 16, d its depth.  Returns the artistic pixel in the same form and
// the depth to store in zout.  `aligned`: the sprite's rows are dword-aligned.
template <int FILTER>
__device__ __forceinline__ uint32_t layer_pixel(const Composite &k, const LayerRow &r, bool aligned, int px, uint32_t o, float d, float &zout) {
    const rtdd_layer &L = k.layer;
    zout = d;
    if (px < k.fx0 || px >= k.fx1) return o;
    // 1. the sprite coordinate
    const uint32_t q = layer_coord(px, L.x, (uint32_t)L.scale);
    if (q >= 256u * (uint32_t)L.cols) return o;
    // 2. the sample
    uint32_t a, cb, cg, cr;
    if (FILTER == RTDD_LAYER_NEAREST) {
        const uint32_t t = texel(r.s0, (int)(q >> 8), aligned);
        cb = t & 255u; cg = (t >> 8) & 255u; cr = (t >> 16) & 255u; a = t >> 24;
    } else {
        const int U = (int)q - 128, iu = U >> 8;
        const uint32_t fu = (uint32_t)(U & 255), fv = r.fv;
        const int t0 = min(max(iu, 0), L.cols - 1), t1 = min(max(iu + 1, 0), L.cols - 1);
        const uint32_t tap[4] = {texel(r.s0, t0, aligned), texel(r.s0, t1, aligned), texel(r.s1, t0, aligned), texel(r.s1, t1, aligned)};
        const uint32_t w[4] = {(256u - fu) * (256u - fv), fu * (256u - fv), (256u - fu) * fv, fu * fv};
        uint32_t A = 0, Cb = 0, Cg = 0, Cr = 0;                     // A <= 65536 * 255, C <= 65536 * 255 * 255 < 2^32
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t wa = w[i] * (tap[i] >> 24);
            A += wa; Cb += wa * (tap[i] & 255u); Cg += wa * ((tap[i] >> 8) & 255u); Cr += wa * ((tap[i] >> 16) & 255u);
        }
        a = (A + 32768u) >> 16;
        if (A) { const uint32_t h = A >> 1; cb = (Cb + h) / A; cg = (Cg + h) / A; cr = (Cr + h) / A; }      // (C + h < 2^32)
        else cb = cg = cr = 0u;
    }
    // 3. the layer's depth
    const int ax = L.x1 - L.x0, ay = L.y1 - L.y0;
    const long long dd = (long long)ax * ax + (long long)ay * ay;   // < 2^31
    float z = L.depth0;
    if (dd) {
        const long long n = min(max((long long)(px - L.x0) * ax + r.ny, 0ll), dd);
        z = L.depth0 + ((L.depth1 - L.depth0) * ((float)(int)n / (float)(int)dd));
    }
    // 4. the visibility
    const float diff = clamp_depth(d) - z;
    uint32_t v;
    if (L.feather == 0.0f) v = diff >= 0.0f ? 256u : 0u;
    else v = (uint32_t)(int)(fminf(fmaxf((diff / L.feather) + 0.5f, 0.0f), 1.0f) * 256.0f);
    // 5. the blend: every product below <= 255 * E + E / 2 < 2^32
    const uint32_t e = a * (uint32_t)L.opacity * v, ne = kLayerE - e;
    const uint32_t ob = (cb * e + (o & 255u) * ne + kLayerE / 2) / kLayerE;
    const uint32_t og = (cg * e + ((o >> 8) & 255u) * ne + kLayerE / 2) / kLayerE;
    const uint32_t orr = (cr * e + ((o >> 16) & 255u) * ne + kLayerE / 2) / kLayerE;
    // 6. the depth
    if (2u * e >= kLayerE) zout = z;
    return ob | (og << 8) | (orr << 16);
}

// VEC: four pixels per lane (rows of both images 4-byte aligned, rows of the depth map -- and of depthOut -- 16-byte aligned).
// DOUT: depthOut is given.
template <int FILTER, bool DOUT, bool VEC>
__global__ __launch_bounds__(256) void k_composite_layer(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                         uint8_t *__restrict__ art, size_t ap, int rows, int cols, Composite k, bool aligned) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform: a wave is one row
    const int lane = threadIdx.x & 63;
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    float *zrow = DOUT ? (float *)((char *)k.depthOut + (size_t)y * k.depthOutPitch) : nullptr;
    const uint8_t *orow = orig + (size_t)y * op;
    uint8_t *arow = art + (size_t)y * ap;
    constexpr int W = VEC ? 256 : 64;                                // pixels of a row a wave covers
    const int xw = blockIdx.x * W;
    // the wave's 1 x W strip against the footprint: scalar
    const bool strip_hits = xw < k.fx1 && xw + W > k.fx0 && y >= k.fy0 && y < k.fy1;
    LayerRow r;
    r.covered = false;
    if (strip_hits) r = layer_row<FILTER>(k, y);
    // one pixel from and to memory: the one-pixel-per-lane path and the ragged end of a vectorised row
    auto pixel = [&](int x) {
        uint32_t o = load_bgr(orow + 3 * (size_t)x);
        float z = drow[x];
        if (r.covered) o = layer_pixel<FILTER>(k, r, aligned, x, o, z, z);
        store_bgr(arow + 3 * (size_t)x, o);
        if (DOUT) zrow[x] = z;
    };
    if (!VEC) {
        const int x = xw + lane;
        if (x < cols) pixel(x);
        return;
    }
    const int x = xw + lane * 4;
    if (x + 3 >= cols) {
        for (int xx = x; xx < cols; xx++) pixel(xx);
        return;
    }
    raw12 o = load_raw<true>(orow, x, cols);
    float4 d4 = *(const float4 *)(drow + x);
    if (r.covered && x < k.fx1 && x + 4 > k.fx0) {
        uint32_t b[12];
        bytes12(o, b);
        float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t p = layer_pixel<FILTER>(k, r, aligned, x + i, b[3 * i] | (b[3 * i + 1] << 8) | (b[3 * i + 2] << 16), dv[i], dv[i]);
            b[3 * i] = p & 255u; b[3 * i + 1] = (p >> 8) & 255u; b[3 * i + 2] = p >> 16;
        }
        store_bytes12(arow + 3 * (size_t)x, b);
        d4 = make_float4(dv[0], dv[1], dv[2], dv[3]);
    } else {
        uint32_t *a3 = (uint32_t *)(arow + 3 * (size_t)x);
        a3[0] = o.w0; a3[1] = o.w1; a3[2] = o.w2;
    }
    if (DOUT) *(float4 *)(zrow + x) = d4;
}

// rtdd_composite_layer (arguments checked and the footprint computed by effects_api.cpp): one launch.
int launch_composite(rtdd_ctx *ctx, const Effect &e) {
    const Composite &k = e.composite;
    const bool dout = k.depthOut != nullptr;
    const bool vec = rows_aligned(e.original, e.originalPitch) && rows_aligned(e.artistic, e.artisticPitch) && rows_aligned(e.depth, e.depthPitch, 16) &&
                     (!dout || rows_aligned(k.depthOut, k.depthOutPitch, 16));
    const bool aligned = rows_aligned(k.sprite, k.spritePitch);
    const bool bilinear = k.layer.filter == RTDD_LAYER_BILINEAR;
    const dim3 g((e.cols + (vec ? 255 : 63)) / (vec ? 256 : 64), (e.rows + 3) / 4);
#define RTDD_CL_LAUNCH(F, D, V) hipLaunchKernelGGL((k_composite_layer<F, D, V>), g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols, k, aligned)
#define RTDD_CL_LAUNCH_V(F, D) do { if (vec) RTDD_CL_LAUNCH(F, D, true); else RTDD_CL_LAUNCH(F, D, false); } while (0)
    if (bilinear) { if (dout) RTDD_CL_LAUNCH_V(RTDD_LAYER_BILINEAR, true); else RTDD_CL_LAUNCH_V(RTDD_LAYER_BILINEAR, false); }
    else { if (dout) RTDD_CL_LAUNCH_V(RTDD_LAYER_NEAREST, true); else RTDD_CL_LAUNCH_V(RTDD_LAYER_NEAREST, false); }
#undef RTDD_CL_LAUNCH_V
#undef RTDD_CL_LAUNCH
    RTDD_LAUNCH_CHECK(ctx, "k_composite_layer");
    return RTDD_OK;
}

}  // namespace rtdd
