// parallax.hip -- the 2-D parallax view (rtdd_simulate_parallax and rtdd_simulate_parallax_layered, include/rtdd.h): the camera moved sideways, up or forward.  Stereo's
// forward warp with a shift in x AND y that may vary over the image (the dolly): sources cross rows, so the occlusion is resolved over
// the whole image, in a z-buffer in global memory, and holes open -- and are filled -- in every direction.
//
// Three stream-ordered passes over one 64-bit key per target (ctx->sat, 8 bytes per pixel):
//   hipMemsetAsync 0xFF    every key all ones: empty
//   k_parallax_scatter     one lane per source: key[t] = min(key[t], bits(d') << 32 | y * cols + x), one no-return 64-bit atomic.  d' is
//                          in [+0, 255]: its bit pattern is non-negative, so unsigned order is depth order; the low word breaks ties
//                          towards the smallest source index and stays below 2^30 (check_effect: rows^2 + cols^2 < 2^31).  The minimum
//                          does not depend on the order of arrival: deterministic.
//   k_parallax_resolve     one lane per target (four where the artistic rows take dword stores): a filled key copies
//                          original[low word]; an empty one marches over the KEYS along the major axis of its own (ax, ay).
// The launch boundary between scatter and resolve is what completes every atomic before a key is read.
//
// Shape.  A wave takes 64 consecutive sources of one row: one 256-byte read of the depth row, and -- neighbouring sources mostly land on
// neighbouring targets -- an atomic wave-instruction that is mostly one or two runs of consecutive 8-byte keys.  The atomics execute
// behind L2, nothing is fetched and nothing returns, so a wave holds no register for them and the kernel keeps full occupancy; what
// bounds it is the rate of atomic requests, not the waves in flight.  No LDS pre-pass (DESIGN.md "Parallax").
//
// The arithmetic is the header's, operation by operation: -ffp-contract=off, no fmaf in this translation unit, `/` correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt): the bytes are those of tests/parallax_ref.py and do not depend on RTDD_OPT_FP_CONTRACT.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

typedef Effect::Parallax Parallax;
constexpr u64 kPxEmpty = ~0ull;

// (ax, ay) of the header at pixel (x, y): the shift of a point 255 depth units behind z0
__device__ __forceinline__ void parallax_a(const Parallax &v, int x, int y, float &ax, float &ay) {
    ax = (float)v.shiftX - (v.dolly * ((float)x - v.cx));
    ay = (float)v.shiftY - (v.dolly * ((float)y - v.cy));
}
// d' with -0 folded into +0 (fmaxf may return either zero): the key's high word is then a non-negative integer
__device__ __forceinline__ float parallax_depth(float d) { return clamp_depth(d) + 0.0f; }

// one source: depth d' = dc, shift field (ax, ay), low word `low`
__device__ __forceinline__ void parallax_put(u64 *__restrict__ keys, int rows, int cols, int x, int y, float ax, float ay, float dc, float z0,
                                             uint32_t low) {
    const float dz = dc - z0;
    const int tx = x + (int)rintf((ax * dz) / 255.0f), ty = y + (int)rintf((ay * dz) / 255.0f);
    if (tx < 0 || tx >= cols || ty < 0 || ty >= rows) return;       // the only stores of the kernel: inside the rows * cols keys
    const u64 key = ((u64)__float_as_uint(dc) << 32) | low;
    (void)__hip_atomic_fetch_min(&keys[(size_t)ty * cols + tx], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_parallax_scatter(const float *__restrict__ depth, size_t dp, u64 *__restrict__ keys, int rows, int cols,
                                                          Parallax v, const float *__restrict__ zp) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform: a wave is 64 sources of one row
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= cols) return;
    const float z0 = zp ? parallax_depth(*zp) : v.zeroDepth;        // the pixel form: one uniform load per wave, when the kernel runs
    const float dc = parallax_depth(((const float *)((const char *)depth + (size_t)y * dp))[x]);
    float ax, ay;
    parallax_a(v, x, y, ax, ay);
    parallax_put(keys, rows, cols, x, y, ax, ay, dc, z0, (uint32_t)(y * cols + x));
}

// pixel `i` (= y * cols + x) of an interleaved BGR image as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t bgr_of_index(const uint8_t *__restrict__ orig, size_t op, uint32_t i, int cols) {
    const uint32_t sy = i / (uint32_t)cols, sx = i - sy * (uint32_t)cols;
    return load_bgr(orig + (size_t)sy * op + 3 * (size_t)sx);
}

// The march of a hole at (x, y) with the step (stx, sty): the key of the first filled target on it and where it stopped, (px, py);
// kPxEmpty when it leaves the image first.  One of |stx|, |sty| is 1: step k is k pixels along the major axis, so at most
// max(rows, cols) - 1 steps stay inside the image.
__device__ __forceinline__ u64 parallax_march(const u64 *__restrict__ keys, int rows, int cols, int x, int y, float stx, float sty, int sign,
                                              int &px, int &py) {
    for (int k = 1;; k++) {
        const float kf = (float)k;
        px = x + sign * (int)rintf(kf * stx); py = y + sign * (int)rintf(kf * sty);
        if (px < 0 || px >= cols || py < 0 || py >= rows) return kPxEmpty;
        const u64 key = keys[(size_t)py * cols + px];
        if (key != kPxEmpty) return key;
    }
}

// A hole at (x, y): the key of the first filled target towards the background side (+a), then towards the other one, and its position
// (px, py); kPxEmpty where neither march meets one (or a == 0: no direction).
__device__ __forceinline__ u64 parallax_hole(const u64 *__restrict__ keys, int rows, int cols, const Parallax &v, int x, int y, int &px, int &py) {
    float ax, ay;
    parallax_a(v, x, y, ax, ay);
    const float m = fmaxf(fabsf(ax), fabsf(ay));
    if (m == 0.0f) return kPxEmpty;
    const float stx = ax / m, sty = ay / m;
    const u64 key = parallax_march(keys, rows, cols, x, y, stx, sty, 1, px, py);
    return key != kPxEmpty ? key : parallax_march(keys, rows, cols, x, y, stx, sty, -1, px, py);
}

// VEC: four targets per lane, the artistic row written as dwords (its rows 4-byte aligned); else one target per lane, written as bytes.
// The original is gathered pixel by pixel either way.
template <bool VEC>
__global__ __launch_bounds__(256) void k_parallax_resolve(const uint8_t *__restrict__ orig, size_t op, const u64 *__restrict__ keys,
                                                          uint8_t *__restrict__ art, size_t ap, int rows, int cols, Parallax v) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform
    const int lane = threadIdx.x & 63;
    uint8_t *arow = art + (size_t)y * ap;
    auto pixel = [&](int x) -> uint32_t {                            // view[(x, y)]
        const uint32_t self = (uint32_t)(y * cols + x);
        u64 key = keys[self];
        int px, py;                                                  // (where a hole's march stopped: not needed here)
        if (key == kPxEmpty) key = parallax_hole(keys, rows, cols, v, x, y, px, py);
        return bgr_of_index(orig, op, key == kPxEmpty ? self : (uint32_t)key, cols);
    };
    if (!VEC) {
        const int x = blockIdx.x * 64 + lane;
        if (x >= cols) return;
        store_bgr(arow + 3 * (size_t)x, pixel(x));
        return;
    }
    const int x = (blockIdx.x * 64 + lane) * 4;
    if (x >= cols) return;
    if (x + 3 < cols) {
        const uint32_t o0 = pixel(x), o1 = pixel(x + 1), o2 = pixel(x + 2), o3 = pixel(x + 3);
        store_bgr4(arow + 3 * (size_t)x, o0, o1, o2, o3);
    } else {
        for (int xx = x; xx < cols; xx++) store_bgr(arow + 3 * (size_t)xx, pixel(xx));     // the ragged end of a row
    }
}

// ---- the two-layer view (rtdd_simulate_parallax_layered) ------------------------------------------------------------------------------
// The same three passes over the same keys; bit 31 of a key's low word says that the source is a plate pixel, so that at equal d' the
// front layer wins and the source index (< 2^30) still breaks the ties within a layer.  The two kernels above are rtdd_simulate_parallax's;
// these are launched when the call has a plate, a depthOut or a coverage.
typedef Effect::ParallaxLayers Layers;
constexpr uint32_t kPxBack = 0x80000000u;

// One lane per pixel, both layers: a wave reads 256 contiguous bytes of each depth row.  A plate source whose d' equals the front's at the
// same pixel lands on the same target with the same high word and the larger low word: it never wins, and no atomic is issued for it
// (d' is never -0 or NaN: equal bits are equal depths).  A plate made by rtdd_remove_object costs atomics on its hole alone.
__global__ __launch_bounds__(256) void k_parallax_scatter_layered(const float *__restrict__ depth, size_t dp, const float *__restrict__ pdepth,
                                                                  size_t pdp, u64 *__restrict__ keys, int rows, int cols, Parallax v,
                                                                  const float *__restrict__ zp) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= cols) return;
    const float z0 = zp ? parallax_depth(*zp) : v.zeroDepth;        // the FRONT map's pixel, for both layers
    const float dc = parallax_depth(((const float *)((const char *)depth + (size_t)y * dp))[x]);
    const float pc = parallax_depth(((const float *)((const char *)pdepth + (size_t)y * pdp))[x]);
    float ax, ay;
    parallax_a(v, x, y, ax, ay);
    const uint32_t self = (uint32_t)(y * cols + x);
    parallax_put(keys, rows, cols, x, y, ax, ay, dc, z0, self);
    if (__float_as_uint(pc) != __float_as_uint(dc)) parallax_put(keys, rows, cols, x, y, ax, ay, pc, z0, self | kPxBack);
}

// The key of the SOURCE of a filled target (x, y) whose own key is `key`: the key itself, unless the target is a crack -- back-won, m != 0,
// and both neighbours p+ and p- of the march's step k = 1 inside the image, front-won and strictly nearer -- which takes p+'s key.  An
// empty key has bit 31 of its low word set: it counts as not front-won.  The high words are non-negative floats: integer order.
__device__ __forceinline__ u64 parallax_source(const u64 *__restrict__ keys, int rows, int cols, const Parallax &v, int x, int y, u64 key) {
    if (!((uint32_t)key & kPxBack)) return key;
    float ax, ay;
    parallax_a(v, x, y, ax, ay);
    const float m = fmaxf(fabsf(ax), fabsf(ay));
    if (m == 0.0f) return key;
    const int dx = (int)rintf(ax / m), dy = (int)rintf(ay / m);      // (rintf(1.0f * st) of the march: the product is exact)
    const int px = x + dx, py = y + dy, qx = x - dx, qy = y - dy;
    if (px < 0 || px >= cols || py < 0 || py >= rows || qx < 0 || qx >= cols || qy < 0 || qy >= rows) return key;
    const u64 kp = keys[(size_t)py * cols + px], kq = keys[(size_t)qy * cols + qx];
    const uint32_t ht = (uint32_t)(key >> 32);
    if ((((uint32_t)kp | (uint32_t)kq) & kPxBack) || (uint32_t)(kp >> 32) >= ht || (uint32_t)(kq >> 32) >= ht) return key;
    return kp;
}

struct PxOut { uint32_t bgr; float d; uint32_t code; };

// VEC: four targets per lane; the rows of artistic and coverage take dword stores, those of depthOut a float4 (every GIVEN output is
// aligned for it); else one target per lane, bytes and single floats.  depthOut and coverage may be null, the plate too (wave-uniform).
template <bool VEC>
__global__ __launch_bounds__(256) void k_parallax_resolve_layered(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth,
                                                                  size_t dp, const uint8_t *__restrict__ plate, size_t pp,
                                                                  const u64 *__restrict__ keys, uint8_t *__restrict__ art, size_t ap,
                                                                  float *__restrict__ dout, size_t zp, uint8_t *__restrict__ cov, size_t cp,
                                                                  int rows, int cols, Parallax v) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;                                           // wave-uniform
    const int lane = threadIdx.x & 63;
    uint8_t *arow = art + (size_t)y * ap;
    float *zrow = dout ? (float *)((char *)dout + (size_t)y * zp) : nullptr;
    uint8_t *crow = cov ? cov + (size_t)y * cp : nullptr;
    auto pixel = [&](int x) -> PxOut {                               // colour, d' and coverage code of view[(x, y)]
        const uint32_t self = (uint32_t)(y * cols + x);
        u64 key = keys[self];
        uint32_t code;
        if (key == kPxEmpty) {                                       // a hole: towards the background side (+a), then the other one
            code = 4;
            int px, py;
            key = parallax_hole(keys, rows, cols, v, x, y, px, py);
            if (key != kPxEmpty) { code = 3; key = parallax_source(keys, rows, cols, v, px, py, key); }     // the hit may be a crack
        } else {
            const u64 s = parallax_source(keys, rows, cols, v, x, y, key);
            code = !((uint32_t)key & kPxBack) ? 0 : (s != key ? 2 : 1);     // (a crack's source is front-won: never the key itself)
            key = s;
        }
        PxOut o;
        o.code = code;
        if (key == kPxEmpty) {                                       // a hole that stays: original[t] and the front d'(t)
            o.bgr = bgr_of_index(orig, op, self, cols);
            o.d = parallax_depth(((const float *)((const char *)depth + (size_t)y * dp))[x]);
        } else {
            const uint32_t low = (uint32_t)key;
            o.bgr = (low & kPxBack) ? bgr_of_index(plate, pp, low & ~kPxBack, cols) : bgr_of_index(orig, op, low, cols);
            o.d = __uint_as_float((uint32_t)(key >> 32));            // the clamped d' with +0, as the scatter packed it
        }
        return o;
    };
    auto store1 = [&](int x, const PxOut &o) {
        store_bgr(arow + 3 * (size_t)x, o.bgr);
        if (zrow) zrow[x] = o.d;
        if (crow) crow[x] = (uint8_t)o.code;
    };
    if (!VEC) {
        const int x = blockIdx.x * 64 + lane;
        if (x >= cols) return;
        store1(x, pixel(x));
        return;
    }
    const int x = (blockIdx.x * 64 + lane) * 4;
    if (x >= cols) return;
    if (x + 3 < cols) {
        const PxOut o0 = pixel(x), o1 = pixel(x + 1), o2 = pixel(x + 2), o3 = pixel(x + 3);
        store_bgr4(arow + 3 * (size_t)x, o0.bgr, o1.bgr, o2.bgr, o3.bgr);
        if (zrow) *(float4 *)(zrow + x) = make_float4(o0.d, o1.d, o2.d, o3.d);
        if (crow) *(uint32_t *)(crow + x) = o0.code | (o1.code << 8) | (o2.code << 16) | (o3.code << 24);
    } else {
        for (int xx = x; xx < cols; xx++) store1(xx, pixel(xx));     // the ragged end of a row
    }
}

// rtdd_simulate_parallax and rtdd_simulate_parallax_layered (arguments checked by effects_api.cpp): the keys emptied, scattered,
// resolved.  A layered call without a plate, a depthOut and a coverage IS rtdd_simulate_parallax: the same launches.
int launch_parallax(rtdd_ctx *ctx, const Effect &e) {
    const Parallax &v = e.parallax;
    const Layers &l = e.layers;
    const bool layered = e.kind == Effect::kParallaxLayered && (l.plate || l.depthOut || l.coverage);
    // The keys live in the context's table buffer.  rows * cols < 2^30 (check_effect), so the buffer stays below 8 GiB and every key
    // index fits the kernels' size_t arithmetic: what can fail is the allocation.
    const size_t npx = (size_t)e.rows * e.cols;
    if (ensure_sat(ctx, npx * 2) != RTDD_OK) {
        (void)hipGetLastError();
        return fail(ctx, RTDD_ERR_NOMEM, "parallax: the key buffer (8 bytes per pixel) could not be allocated");
    }
    ctx->sat_rows = ctx->sat_cols = 0;                               // whatever table lay here is gone: the next table-path defocus zeroes its padding again
    u64 *keys = (u64 *)ctx->sat;
    RTDD_HIP(ctx, hipMemsetAsync(keys, 0xFF, npx * sizeof(u64), ctx->stream));
    const float *zp = pixel_ptr(e.depth, e.depthPitch, v.zeroX, v.zeroY);     // the pixel form of z0: the FRONT map's
    const dim3 g((e.cols + 63) / 64, (e.rows + 3) / 4), g4((e.cols + 255) / 256, g.y);
    if (layered && l.plate) {
        hipLaunchKernelGGL(k_parallax_scatter_layered, g, dim3(256), 0, ctx->stream, e.depth, e.depthPitch, l.plateDepth, l.plateDepthPitch, keys,
                           e.rows, e.cols, v, zp);
        RTDD_LAUNCH_CHECK(ctx, "k_parallax_scatter_layered");
    } else {
        hipLaunchKernelGGL(k_parallax_scatter, g, dim3(256), 0, ctx->stream, e.depth, e.depthPitch, keys, e.rows, e.cols, v, zp);
        RTDD_LAUNCH_CHECK(ctx, "k_parallax_scatter");
    }
    if (layered) {
        const bool vec = rows_aligned(e.artistic, e.artisticPitch) && (!l.depthOut || rows_aligned(l.depthOut, l.depthOutPitch, 16)) &&
                         (!l.coverage || rows_aligned(l.coverage, l.coveragePitch));
        if (vec)
            hipLaunchKernelGGL(k_parallax_resolve_layered<true>, g4, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch,
                               l.plate, l.platePitch, keys, e.artistic, e.artisticPitch, l.depthOut, l.depthOutPitch, l.coverage, l.coveragePitch,
                               e.rows, e.cols, v);
        else hipLaunchKernelGGL(k_parallax_resolve_layered<false>, g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch,
                                l.plate, l.platePitch, keys, e.artistic, e.artisticPitch, l.depthOut, l.depthOutPitch, l.coverage, l.coveragePitch,
                                e.rows, e.cols, v);
        RTDD_LAUNCH_CHECK(ctx, "k_parallax_resolve_layered");
        return RTDD_OK;
    }
    if (rows_aligned(e.artistic, e.artisticPitch))
        hipLaunchKernelGGL(k_parallax_resolve<true>, g4, dim3(256), 0, ctx->stream, e.original, e.originalPitch, keys, e.artistic, e.artisticPitch,
                           e.rows, e.cols, v);
    else hipLaunchKernelGGL(k_parallax_resolve<false>, g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, keys, e.artistic, e.artisticPitch,
                            e.rows, e.cols, v);
    RTDD_LAUNCH_CHECK(ctx, "k_parallax_resolve");
    return RTDD_OK;
}

}  // namespace rtdd
