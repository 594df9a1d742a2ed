// effect_kernels.hip -- depth-driven artistic passes (desaturation, haze, defocus).
//
// Desaturation and haze are pure streaming (11 / 10 B per pixel).  A thread handles FOUR pixels so
// the interleaved u8x3 rows move as dwordx3 (12 B/lane, contiguous across the wave) and depth as
// dwordx4, instead of the reference's one-thread-per-pixel byte accesses
// (/root/reference/src/GPUDepthEffect.cu:18-25, 83-91); rows that are not 4-byte aligned take a
// byte-wise path with identical arithmetic.
//
// Defocus in the reference is a per-pixel O(k^2) gather (up to 48 400 taps at 8K, src/GPUDepthEffect.cu:47-60); here it is an
// exact O(1) lookup in a packed 64-bit summed-area table written once -- see "defocus" below.
#include "rtdd_internal.hpp"
#include "persist_sync.hpp"
#include "effect_common.hpp"

namespace rtdd {

// simulateDesaturation (K8) -- src/GPUDepthEffect.cu:8-27
template <bool CONTRACT>
__device__ __forceinline__ uint32_t desat_px(float d, float g, float o) {
    const float f = (float)((double)d / 255.0);                    // :22 (double divide, narrowed)
    const float t = (1 - f) * o;
    return store_u8(CONTRACT ? __builtin_fmaf(f, g, t) : f * g + t);
}

// simulateHaze (K10) -- src/GPUDepthEffect.cu:74-93.  exp by the SAME fixed sequence of IEEE f64 operations as the CPU restatement's
// deterministic exp (the test infrastructure's a12 section: the same literals, the same fma chain, one rounding to f32, no libm on either side), so the
// transmission t -- and with it every output byte -- is bit-identical to the restatement's.  (CUDA's device expf, which the
// reference calls, is a <= 2 ulp libdevice routine and not reproducible anywhere; this one is faithful to < 0.5000001 ulp.)
__device__ __forceinline__ float expf_det(float x) {
    if (x != x) return x;
    if (x > 89.0f) return __builtin_inff();
    if (x < -104.0f) return 0.0f;                                   // exp(-104) < 2^-150: rounds to 0
    const double xd = (double)x;
    const double kd = __builtin_rint(xd * 0x1.71547652b82fep+0);
    const double r = __builtin_fma(-kd, 0x1.a39ef35793c76p-33, __builtin_fma(-kd, 0x1.62e42fee00000p-1, xd));
    double p = 0x1.6124613a86d09p-33;                               // 1/13! ... 1/2!
    p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29); p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26); p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);
    p = __builtin_fma(p, r, 0x1.71de3a556c734p-19); p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16); p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);
    p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10); p = __builtin_fma(p, r, 0x1.1111111111111p-7); p = __builtin_fma(p, r, 0x1.5555555555555p-5);
    p = __builtin_fma(p, r, 0x1.5555555555555p-3); p = __builtin_fma(p, r, 0x1.0000000000000p-1); p = __builtin_fma(p, r, 1.0); p = __builtin_fma(p, r, 1.0);
    const double s = __builtin_bit_cast(double, (unsigned long long)((int)kd + 1023) << 52);      // 2^k, k in [-151, 129]
    return (float)(p * s);
}
__device__ __forceinline__ float haze_t(float d) {
    const float arg = (float)((double)(-2.0f * d) / 255.0);        // :88
    return expf_det(arg);
}
template <bool CONTRACT>
__device__ __forceinline__ uint32_t haze_px(float t, float w, float o) {
    return store_u8(CONTRACT ? __builtin_fmaf(t, o, w) : t * o + w);
}
// rtdd_simulate_haze_ex: :88 with the density beta a parameter; the airlight replaces the 255 of :89-91 per channel
__device__ __forceinline__ float haze_t_beta(float d, float beta) {
    return expf_det((float)((double)(-beta * d) / 255.0));
}

// MODE 0 = desaturation, 1 = haze, 2 = haze with density `beta` and airlight `air` (b | g << 8 | r << 16; modes 0 and 1 ignore both).
// VEC: 4 pixels per thread with dword accesses (needs 4-byte aligned rows).
template <int MODE, bool CONTRACT, bool VEC>
__global__ __launch_bounds__(256) void k_blend(const uint8_t *__restrict__ orig, size_t op, const uint8_t *__restrict__ gray, size_t gp,
                                               const float *__restrict__ depth, size_t dp, uint8_t *__restrict__ art, size_t ap,
                                               int rows, int cols, float beta, uint32_t air) {
    const int y = blockIdx.y * 4 + wave_id();
    if (y >= rows) return;
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const uint8_t *orow = orig + (size_t)y * op;
    uint8_t *arow = art + (size_t)y * ap;
    const float airf[3] = {(float)(air & 255), (float)((air >> 8) & 255), (float)((air >> 16) & 255)};
    if (VEC) {
        const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
        if (x + 3 < cols) {
            const float4 d4 = *(const float4 *)(drow + x);
            const uint32_t *o3 = (const uint32_t *)(orow + 3 * x);
            const raw12 o = {o3[0], o3[1], o3[2]};
            uint32_t g4 = 0;
            if (MODE == 0) g4 = *(const uint32_t *)(gray + (size_t)y * gp + x);
            const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
            uint32_t ob[12], rb[12];
            bytes12(o, ob);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (MODE == 0) {
                    const float g = (float)((g4 >> (8 * i)) & 255);
#pragma unroll
                    for (int c = 0; c < 3; c++) rb[3 * i + c] = desat_px<CONTRACT>(dv[i], g, (float)ob[3 * i + c]);
                } else if (MODE == 1) {
                    const float t = haze_t(dv[i]);
                    const float w = (1 - t) * 255;
#pragma unroll
                    for (int c = 0; c < 3; c++) rb[3 * i + c] = haze_px<CONTRACT>(t, w, (float)ob[3 * i + c]);
                } else {
                    const float t = haze_t_beta(dv[i], beta), u = 1 - t;
#pragma unroll
                    for (int c = 0; c < 3; c++) rb[3 * i + c] = haze_px<CONTRACT>(t, u * airf[c], (float)ob[3 * i + c]);
                }
            }
            store_bytes12(arow + 3 * x, rb);
            return;
        }
        // ragged tail of a vectorised row: fall through to the scalar body for the remaining pixels
        for (int xx = x; xx < cols; xx++) {
            const float d = drow[xx];
            if (MODE == 0) { const float g = (float)gray[(size_t)y * gp + xx];
                for (int c = 0; c < 3; c++) arow[3 * xx + c] = (uint8_t)desat_px<CONTRACT>(d, g, (float)orow[3 * xx + c]); }
            else if (MODE == 1) { const float t = haze_t(d); const float w = (1 - t) * 255;
                for (int c = 0; c < 3; c++) arow[3 * xx + c] = (uint8_t)haze_px<CONTRACT>(t, w, (float)orow[3 * xx + c]); }
            else { const float t = haze_t_beta(d, beta), u = 1 - t;
                for (int c = 0; c < 3; c++) arow[3 * xx + c] = (uint8_t)haze_px<CONTRACT>(t, u * airf[c], (float)orow[3 * xx + c]); }
        }
    } else {
        const int x = blockIdx.x * 64 + (threadIdx.x & 63);
        if (x >= cols) return;
        const float d = drow[x];
        if (MODE == 0) { const float g = (float)gray[(size_t)y * gp + x];
#pragma unroll
            for (int c = 0; c < 3; c++) arow[3 * x + c] = (uint8_t)desat_px<CONTRACT>(d, g, (float)orow[3 * x + c]); }
        else if (MODE == 1) { const float t = haze_t(d); const float w = (1 - t) * 255;
#pragma unroll
            for (int c = 0; c < 3; c++) arow[3 * x + c] = (uint8_t)haze_px<CONTRACT>(t, w, (float)orow[3 * x + c]); }
        else { const float t = haze_t_beta(d, beta), u = 1 - t;
#pragma unroll
            for (int c = 0; c < 3; c++) arow[3 * x + c] = (uint8_t)haze_px<CONTRACT>(t, u * airf[c], (float)orow[3 * x + c]); }
    }
}

// ---- stereo: a per-row forward warp (rtdd_simulate_stereo, include/rtdd.h) -----------------------------------------------------
// Source x lands on target x + s(x), s = (int)rintf((D * (d' - z0)) / 255) in f32 with no fused operation (|s| <= |D| <= 256); the
// nearest source (smallest s * sign(D)) wins a target; a hole copies the view of the nearest filled target on the background side, else
// of the other side, else original[t].  One workgroup per (row, segment of kStW targets); no global atomics, no communication between
// workgroups.  Halo (DESIGN.md "Stereo"): every hole run that is not the whole row is at most |D| + 1 long, so a hole's filled
// neighbours on both sides lie within H = |D| + 1 of it -- the workgroup resolves the targets [t0 - H, t1 + H) (E), and those are
// reached only from the sources [t0 - H - |D|, t1 + H + |D|).  A row with no filled target has cols <= |D| + 1 <= H: E is the whole row.
constexpr int kStMaxD = 256, kStW = 1024, kStMaxE = kStW + 2 * (kStMaxD + 1), kStC = (kStMaxE + 255) / 256;
constexpr uint32_t kStEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ int stereo_shift(float d, float z0, float D) {
    return (int)rintf((D * (clamp_depth(d) - z0)) / 255.0f);                    // (-ffp-contract=off, IEEE divide: three roundings)
}
// pixel x of an interleaved BGR row as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t bgr_at(const uint8_t *row, int x) { return load_bgr(row + 3 * (size_t)x); }

// VEC: 4 targets per thread with dword accesses (needs 4-byte aligned rows of the original and the artistic image).  zp: the depth
// map's zero-parallax pixel (the pixel form, read here when the kernel runs), else z0 is the value `zval`.
template <bool VEC>
__global__ __launch_bounds__(256) void k_stereo(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                uint8_t *__restrict__ art, size_t ap, int rows, int cols, int D, float zval,
                                                const float *__restrict__ zp, int anaglyph) {
    __shared__ uint32_t key[kStMaxE];                               // per target of E: sign(D) * s + 256 of the winner (kStEmpty: a hole)
    __shared__ int res[kStW];                                       // per target of the segment: the source whose colour it takes (-1: original[t])
    __shared__ int wl[4], wr[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int y = blockIdx.y, t0 = blockIdx.x * kStW, t1 = min(cols, t0 + kStW);
    const int aD = D < 0 ? -D : D, sg = D < 0 ? -1 : 1, H = aD + 1;
    const int e0 = max(0, t0 - H), e1 = min(cols, t1 + H), nE = e1 - e0;
    const float z0 = zp ? clamp_depth(*zp) : zval;
    const float Df = (float)D;
    const float *drow = (const float *)((const char *)depth + (size_t)y * dp);
    const uint8_t *orow = orig + (size_t)y * op;
    uint8_t *arow = art + (size_t)y * ap;

    for (int i = tid; i < nE; i += 256) key[i] = kStEmpty;
    __syncthreads();
    // every source that can land in E; the minimum key picks the nearest (equal shifts never share a target: no ties)
    for (int x = max(0, e0 - aD) + tid, xe = min(cols, e1 + aD); x < xe; x += 256) {
        const int s = stereo_shift(drow[x], z0, Df), t = x + s;
        if (t >= e0 && t < e1) atomicMin(&key[t - e0], (uint32_t)(sg * s + 256));
    }
    __syncthreads();

    // nearest filled slot at or left of (lf) and at or right of (rf) every slot: thread chunks of kStC slots, a max / min scan over them
    const int c0 = tid * kStC;
    int last = -1, first = 0x7FFFFFFF;
#pragma unroll
    for (int i = 0; i < kStC; i++) {
        const int j = c0 + i;
        if (j < nE && key[j] != kStEmpty) { last = j; if (first == 0x7FFFFFFF) first = j; }
    }
    int a = last, b = first;                                        // inclusive scans within the wave: max from the left, min from the right
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(a, o), v = __shfl_down(b, o);
        if (lane >= o) a = max(a, u);
        if (lane + o < 64) b = min(b, v);
    }
    if (lane == 63) wl[w] = a;
    if (lane == 0) wr[w] = b;
    int exl = __shfl_up(a, 1), exr = __shfl_down(b, 1);
    if (lane == 0) exl = -1;
    if (lane == 63) exr = 0x7FFFFFFF;
    __syncthreads();
    for (int k = 0; k < w; k++) exl = max(exl, wl[k]);
    for (int k = w + 1; k < 4; k++) exr = min(exr, wr[k]);
    int lf[kStC];
#pragma unroll
    for (int i = 0; i < kStC; i++) {
        const int j = c0 + i;
        if (j < nE && key[j] != kStEmpty) exl = j;
        lf[i] = exl;
    }
#pragma unroll
    for (int i = kStC - 1; i >= 0; i--) {
        const int j = c0 + i;
        if (j >= nE) continue;
        if (key[j] != kStEmpty) exr = j;
        const int t = e0 + j;
        if (t < t0 || t >= t1) continue;
        const int rf = exr == 0x7FFFFFFF ? -1 : exr;
        const int pick = D > 0 ? (rf >= 0 ? rf : lf[i]) : (lf[i] >= 0 ? lf[i] : rf);     // the background side first (filled: itself)
        res[t - t0] = pick < 0 ? -1 : (e0 + pick) - sg * ((int)key[pick] - 256);
    }
    __syncthreads();

    const int tb = t0 + 4 * tid;
    if (tb >= t1) return;
    uint32_t out[4];
    const bool whole = VEC && tb + 3 < t1;
    uint32_t ow[3] = {0, 0, 0};
    if (whole && anaglyph) { const uint32_t *o3 = (const uint32_t *)(orow + 3 * (size_t)tb); ow[0] = o3[0]; ow[1] = o3[1]; ow[2] = o3[2]; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int t = tb + i;
        if (t >= t1) break;
        const int x = res[t - t0];
        uint32_t v = bgr_at(orow, x >= 0 ? x : t);
        if (anaglyph) {
            uint32_t o;
            if (whole) {
                const uint32_t lo = i == 0 ? ow[0] : i == 1 ? (ow[0] >> 24) | (ow[1] << 8) : i == 2 ? (ow[1] >> 16) | (ow[2] << 16) : ow[2] >> 8;
                o = lo & 0xFFFFFFu;
            } else {
                o = bgr_at(orow, t);
            }
            v = D >= 0 ? (v & 0x00FFFFu) | (o & 0xFF0000u) : (o & 0x00FFFFu) | (v & 0xFF0000u);   // (view.b, view.g, orig.r) | (orig.b, orig.g, view.r)
        }
        out[i] = v;
    }
    if (whole) {
        store_bgr4(arow + 3 * (size_t)tb, out[0], out[1], out[2], out[3]);
    } else {
        for (int i = 0; i < 4 && tb + i < t1; i++) store_bgr(arow + 3 * (size_t)(tb + i), out[i]);
    }
}

// ---- defocus: packed summed-area table ---------------------------------------------------------------
// The reference gathers up to (2*(K/2))^2 taps per pixel (src/GPUDepthEffect.cu:47-60: 2 916 at 1080p, 12 100 at 4K, 48 400 at 8K).
// Here: an exact O(1) lookup.  A pixel is packed into ONE 64-bit integer  p = B + G * 2^21 + R * 2^42  and
//     T[r][c] = sum of p over rows <= r, columns <= c          (plain 64-bit adds, i.e. arithmetic mod 2^64)
// is stored once, 8 aligned bytes per pixel.  Any rectangle sum  X = T(y1,x1) - T(y1,x0) - T(y0,x1) + T(y0,x0)  (mod 2^64) is the
// packed integer of its three channel sums; whenever each of those is < 2^21 -- a window of at most kSatMaxArea = 8224 pixels,
// 8224 * 255 < 2^21 -- the fields do not run into each other and B, G, R are read off X exactly (carries between the fields of the
// PREFIXES cancel: Z/2^64 is a ring).  Larger windows (12 100 px at 4K, 48 400 at 8K, or an out-of-range depth) are cut into
// horizontal strips of <= 8224 px that share corner rows: n strips cost 2 (n + 1) loads.  The channel sums are < 2^24 for every
// nominal window, so the reference's f32 accumulation is exact and so is the u32 -> f32 conversion here: bit-identical results.
// Round 2 kept 12-byte {B,G,R} u32 entries written by a row pass, rewritten by a band pass, and read 8 times per pixel (table + band
// base at four corners, unaligned): 60-130 B/px moved against 10 B/px algorithmic.
//
// Build, three launches, the table written exactly once:
//   k_sat_colsum   per band of RB rows and per column: packed sum of the band's pixels                  (reads the image: 3 B/px)
//   k_sat_colbase  exclusive scan of those sums down the bands, per column (tiny: rows/RB x cols x 8 B)
//   k_sat_build    one workgroup per band, the full row width: running column sums from the band's base, row prefix by a 64-bit
//                  DPP wave scan + one LDS exchange of wave totals per four rows, one aligned 32-byte store per four pixels
// and k_defocus reads its four (or 2 (n + 1)) corners with aligned 8-byte loads.
// pass 1: colsum[band][x] = packed sum of the pixels of column x in rows [band*RB, band*RB + RB).  A thread owns four columns;
// eight rows of loads are in flight at a time.
template <bool VEC>
__global__ __launch_bounds__(256) void k_sat_colsum(const uint8_t *__restrict__ orig, size_t op, u64 *__restrict__ colsum, int tp, int rows, int cols, int RB) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, band = blockIdx.y;
    if (x >= tp) return;
    const int ra = band * RB, rb = min(ra + RB, rows);
    u64 s[4] = {0, 0, 0, 0};
    for (int r = ra; r < rb; r += 8) {
        raw12 v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = load_raw<VEC>(orig + (size_t)min(r + i, rb - 1) * op, x, cols);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            u64 px[4];
            unpack4(v[i].w0, v[i].w1, v[i].w2, px);
            if (r + i < rb) { s[0] += px[0]; s[1] += px[1]; s[2] += px[2]; s[3] += px[3]; }
        }
    }
    u64x2 *out = (u64x2 *)(colsum + (size_t)band * tp + x);
    out[0] = u64x2{s[0], s[1]}; out[1] = u64x2{s[2], s[3]};
}

// pass 2: in place, colsum[band][x] -> sum of colsum[b][x] over b < band.  One workgroup per 64 columns (lane = column); its waves
// split the bands (at most kScanChunk each, all loads in flight), trade totals through LDS, and write their share's exclusive prefixes.
constexpr int kScanChunk = 32;
__global__ __launch_bounds__(1024) void k_sat_colbase(u64 *__restrict__ colsum, int tp, int nbands) {
    __shared__ u64 tot[16][64];
    const int lane = threadIdx.x & 63, w = wave_id(), nw = (int)blockDim.x >> 6;
    const int x = min(blockIdx.x * 64 + lane, tp - 1);             // (the last workgroup's spare lanes repeat column tp-1: same values, same stores)
    const int chunk = min((nbands + nw - 1) / nw, kScanChunk);      // bands per wave and round
    u64 carry = 0;                                                  // bands before this round of nw * chunk
    for (int b0 = 0; b0 < nbands; b0 += nw * chunk) {
        const int ba = min(b0 + w * chunk, nbands), bb = min(ba + chunk, nbands);
        u64 v[kScanChunk], sum = 0;
#pragma unroll
        for (int i = 0; i < kScanChunk; i++) v[i] = ba + i < bb ? colsum[(size_t)(ba + i) * tp + x] : 0ull;
#pragma unroll
        for (int i = 0; i < kScanChunk; i++) sum += v[i];
        __syncthreads();                                            // (tot may still be read from the round before)
        tot[w][lane] = sum;
        __syncthreads();
        u64 run = carry, all = 0;
        for (int k = 0; k < nw; k++) { const u64 t = tot[k][lane]; all += t; if (k < w) run += t; }
        carry += all;
#pragma unroll
        for (int i = 0; i < kScanChunk; i++) if (ba + i < bb) { colsum[(size_t)(ba + i) * tp + x] = run; run += v[i]; }
    }
}

// pass 3: the table.  Workgroup = band of RB rows x the full row width, 4 consecutive pixels per thread (so a wave covers 256
// pixels and rows up to 4096 pixels need ONE sweep of the row; wider rows loop over column ranges with a per-row carry in LDS).
// Four rows at a time, the next four rows' loads already in flight: running column sums col[j] (they start at the band's base),
// in-thread prefix over the 4 pixels, 64-bit wave scan of the thread totals, wave totals to LDS, ONE barrier, prefix of the <= 16
// wave totals by a 16-lane scan, two aligned 16-byte stores per row.
template <bool VEC>
__global__ __launch_bounds__(1024) void k_sat_build(const uint8_t *__restrict__ orig, size_t op, const u64 *__restrict__ colbase, u64 *__restrict__ T,
                                                    int tp, int rows, int cols, int RB, int tpitch) {
    __shared__ u64 wtot[2][4][16];                                  // [buffer][row of the group of four][wave]
    __shared__ u64 rowcarry[2][32];                                 // [parity of the column range][row of the band]: everything left of the range
    const int tid = threadIdx.x, lane = tid & 63, nt = (int)blockDim.x, nw = nt >> 6;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int band = blockIdx.x, r0 = band * RB;
    if (tid < 64) rowcarry[tid >> 5][tid & 31] = 0;
    __syncthreads();
    int buf = 0, par = 0;
    for (int x0 = 0; x0 < cols; x0 += nt * 4, par ^= 1) {
        const int x = x0 + tid * 4;
        u64 col[4] = {0, 0, 0, 0};
        raw12 nxt[4];
#pragma unroll
        for (int i = 0; i < 4; i++) nxt[i] = load_raw<VEC>(orig + (size_t)min(r0 + i, rows - 1) * op, x, cols);
        if (x < tp) {
            const u64x2 *q = (const u64x2 *)(colbase + (size_t)band * tp + x);
            const u64x2 a = q[0], b = q[1];
            col[0] = a.a; col[1] = a.b; col[2] = b.a; col[3] = b.b;
        }
        for (int sub = 0; sub < RB; sub += 4, buf ^= 1) {
            raw12 cur[4];
#pragma unroll
            for (int i = 0; i < 4; i++) cur[i] = nxt[i];
            if (sub + 4 < RB) {
#pragma unroll
                for (int i = 0; i < 4; i++) nxt[i] = load_raw<VEC>(orig + (size_t)min(r0 + sub + 4 + i, rows - 1) * op, x, cols);
            }
            u64 s[4][4], excl[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                u64 px[4];
                unpack4(cur[i].w0, cur[i].w1, cur[i].w2, px);
                if (r0 + sub + i < rows) {                          // (rows past the image: never stored; the band ends with them)
#pragma unroll
                    for (int j = 0; j < 4; j++) col[j] += px[j];
                }
                s[i][0] = col[0]; s[i][1] = s[i][0] + col[1]; s[i][2] = s[i][1] + col[2]; s[i][3] = s[i][2] + col[3];
                const u64 incl = wave_incl_scan64(s[i][3]);
                excl[i] = incl - s[i][3];
                if (lane == 63) wtot[buf][i][w] = incl;             // the wave's total of row i
            }
            __syncthreads();
            // lanes 16 i .. 16 i + 15 take row i's wave totals: ONE 16-lane scan serves the four rows
            const u64 t = (lane & 15) < nw ? wtot[buf][lane >> 4][lane & 15] : 0;
            const u64 inc = row16_incl_scan64(t), exc = inc - t;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = r0 + sub + i;
                const u64 before = readlane64(exc, 16 * i + w), all = readlane64(inc, 16 * i + nw - 1);
                const u64 left = rowcarry[par][sub + i];
                const u64 add = left + before + excl[i];
                if (r < rows && x < tp) {
                    u64x2 *q = (u64x2 *)(T + (size_t)r * tpitch + x);
                    q[0] = u64x2{s[i][0] + add, s[i][1] + add}; q[1] = u64x2{s[i][2] + add, s[i][3] + add};
                }
                if (tid == 0) rowcarry[par ^ 1][sub + i] = left + all;   // read again only after the next barrier
            }
        }
    }
}

// k / 2 of  int k = kernelSize * depth / 255.0  (src/GPUDepthEffect.cu:43: int * float -> float, / double, truncation), without the
// f64 divide.  v = (float)kernelSize * depth is an f32, so the double quotient v / 255.0 never rounds across an integer (a non-integer
// exact quotient is at least 2^-24 relative away from one, the rounding error is 2^-53) and (int) of it is floor(v / 255) exactly:
// q0 = v * (1/255) is within 1 of it, the remainder v - 255 k0 is exact in f32 for v >= 256, one correction step.  v < 510 (k < 2),
// negative and NaN products give a half-width <= 0: the reference's loops do not run and the pixel is copied (0 returned here).
// Products beyond 255 * 2^22 are clamped: any k/2 >= max(rows, cols) selects the whole (clipped) image anyway.
__device__ __forceinline__ int half_window(int kernelSize, float d) {
    const float v0 = (float)kernelSize * d;
    const float v = __builtin_amdgcn_fmed3f(v0, 0.0f, 1069547520.0f);   // 255 * 2^22 (a NaN gives 0); straight-line code: the table loads that depend on it issue sooner
    int k = (int)(v * (1.0f / 255.0f));
    const float r = __builtin_fmaf(-255.0f, (float)k, v);           // exact
    k += r < 0.0f ? -1 : (r >= 255.0f ? 1 : 0);
    return v0 >= 510.0f ? k >> 1 : 0;                               // <= 2^21
}

// simulateDefocus (K9) -- src/GPUDepthEffect.cu:29-72: the lookup.  Lane = pixel, wave = 64 pixels x 2 rows, workgroup = 64 x 8 pixels
// (1 / 2 / 4 / 8 rows per wave measured 50.8 / 48.2 / 55.7 / 75.0 us at 4K in round 3: a wave that spreads over more rows keeps fewer of
// the table lines it gathers in L1 between its left- and right-corner loads; TWO pixels per lane in x measured 101 against 79 us in
// round 5 -- a wave instruction then touches twice the lines).  Workgroups are numbered so that each XCD (dispatch: workgroup p -> XCD
// p % 8) takes a contiguous band of tile rows.  Round 5 rebuilt the kernel around its instruction count and its loads:
//   * the table is PADDED: one zero row above row 0 and four zero entries left of column 0 (T'[r + 1][c + 4] = T(r, c); the padding is
//     zeroed when the table's geometry changes and nobody ever writes it), so T(-1, .) = T(., -1) = 0 needs no select;
//   * the four corners are raw BUFFER loads: a 32-bit byte offset each -- row * pitch_bytes is one 24-bit multiply shared by two
//     corners, the column term one shift-add shared by two -- instead of four 64-bit address computations with a select each;
//   * the original pixel is only needed where the window is empty (depth < 510 / kernelSize: the reference's loops do not run and the
//     pixel is copied): loaded under one wave-uniform branch, not for every pixel (25 MB less at 4K);
//   * `art` moves as dwords: the three dwords of a quad of pixels are stored by its first three lanes after one quad permute.
// 4K smooth depth 86.5 -> 78.5 us for the whole effect, 1440p 46.0 -> 43.2, 8K 746 -> 732 (profiles/r05_defocus_lookup_ab.txt); the
// same integer sums and quotient code as before: bit-identical (every pixel at 4K / 8K against an independent table, tests/).
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u64 tab_load(__amdgpu_buffer_rsrc_t rsrc, uint32_t byte_off) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, byte_off, 0, 0);
    return ((u64)v.y << 32) | v.x;
}

constexpr int kLk2Rows = 2;                                         // rows per wave
template <bool VEC, bool FOCUS>
__global__ __launch_bounds__(256) void k_defocus(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                  const u64 *__restrict__ Tpad, int tpitch, uint8_t *__restrict__ art, size_t ap,
                                                  int rows, int cols, int kernelSize, int gx, int ntiles, int xcd_tiles,
                                                  int row0, int row1, int trow0, int trows, int *__restrict__ nonlocal_word, int strip_w,
                                                  float focus, const float *__restrict__ focus_px) {
    // Round 6, BANDED tables (defocus_body): this launch writes output rows [row0, row1) and the table holds image rows
    // [trow0, trow0 + trows) with its origin at row trow0 -- rectangle sums are differences, so any origin above the window serves.  The
    // whole image in one launch: row0 = trow0 = 0, row1 = trows = rows.
    // Which tile: workgroup p is dispatched to XCD p % 8.  strip_w == 0: each XCD takes a contiguous band of tile ROWS.  strip_w > 0
    // (round 6, wide images): each XCD takes a COLUMN strip strip_w tiles wide and walks it row by row -- a table line read as a window's
    // bottom edge is read again as a top edge 2 h rows later, and only a strip's 2 h rows (8K: 220 x 960 px x 8 B = 1.7 MB), not the
    // whole image width's (13.5 MB), fit the XCD's 4 MB L2 in between.
    int tx, ty;
    if (!tile_of_workgroup(blockIdx.x, gx, ntiles, xcd_tiles, strip_w, tx, ty)) return;
    const int lane = threadIdx.x & 63, wv = wave_id();
    const int x0 = tx * 64, yw = row0 + ty * (4 * kLk2Rows) + wv * kLk2Rows;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)Tpad, 0, (int)((uint32_t)(trows + 1) * (uint32_t)tpitch * 8u), 0x00020000);
    const uint32_t pitch8 = (uint32_t)tpitch * 8u;
    const bool whole = VEC && x0 + 64 <= cols;                      // wave-uniform: the output as dwords
    const int x = x0 + lane, xc = min(x, cols - 1);
    float d[kLk2Rows];
#pragma unroll
    for (int i = 0; i < kLk2Rows; i++) d[i] = ((const float *)((const char *)depth + (size_t)min(yw + i, rows - 1) * dp))[xc];
    if (FOCUS) {
        const float f = focal_depth(focus, focus_px);
#pragma unroll
        for (int i = 0; i < kLk2Rows; i++) d[i] = fabsf(d[i] - f);
    }
    uint32_t cnt[kLk2Rows];
    u64 C[kLk2Rows][4];
    int ya[kLk2Rows], yb[kLk2Rows], xa[kLk2Rows], xb[kLk2Rows];
#pragma unroll
    for (int i = 0; i < kLk2Rows; i++) {                            // every corner load of the wave's rows before the first is used
        const int y = min(yw + i, rows - 1);
        const int h = half_window(kernelSize, d[i]);                // <= 2^21: y + h stays an int
        ya[i] = max(y - h, 0); yb[i] = min(y + h, rows);
        xa[i] = max(xc - h, 0); xb[i] = min(xc + h, cols);
        // T(ya - 1, xa - 1) = T'[ya][xa + 3], ...: byte offsets row * pitch8 + 8 * col + 24 (rows counted from the table's origin row)
        const uint32_t ra = (uint32_t)__umul24(ya[i] - trow0, pitch8), rb = (uint32_t)__umul24(yb[i] - trow0, pitch8);       // both factors < 2^24 and (rows + 1) * pitch8 < 2^32: defocus_body refuses any larger table
        const uint32_t ca = 8u * (uint32_t)xa[i] + 24u, cb = 8u * (uint32_t)xb[i] + 24u;
        C[i][0] = tab_load(rsrc, ra + ca); C[i][1] = tab_load(rsrc, ra + cb); C[i][2] = tab_load(rsrc, rb + ca); C[i][3] = tab_load(rsrc, rb + cb);
        const int wd = xb[i] - xa[i], ht = yb[i] - ya[i];
        cnt[i] = (wd > 0 && ht > 0) ? (uint32_t)__umul24(ht, wd) : 0u;   // (both < 2^16: rows^2 + cols^2 < 2^31, check_effect)
    }
#pragma unroll
    for (int i = 0; i < kLk2Rows; i++) {
        const int y = yw + i, yc = min(y, rows - 1);
        uint32_t res;
        {
            const u64 X = C[i][3] - C[i][2] - C[i][1] + C[i][0];
            const uint32_t lo = (uint32_t)X, hi = (uint32_t)(X >> 32);
            const uint32_t sb = lo & (uint32_t)kSatFieldMask, sg = ((lo >> 21) | (hi << 11)) & (uint32_t)kSatFieldMask, sr = hi >> 10;
            const uint32_t c = cnt[i] ? cnt[i] : 1u;
            res = quot3_u8(sb, sg, sr, c, __builtin_amdgcn_rcpf((float)c));
        }
        // windows of more than kSatMaxArea pixels (the packed fields would run into each other) and empty ones: under wave-uniform branches.
        // Such a window is cut into horizontal strips of <= kSatMaxArea pixels that share corner rows.  Round 6: its first and last corner
        // rows are the four corners already in hand, so n strips cost 2 (n - 1) more loads, not 2 (n + 1) -- two instead of six for the
        // two strips of a 4K window, ten instead of fourteen for the six of an 8K one; the lookup is bound by the table lines its load
        // instructions pull through L1 (only the lanes WITH a large window issue them: walking the strips in lock step with loads two
        // rows ahead, all lanes together, was built and is slower -- 8K random 1342 -> 2104 us -- see EXPERIMENTS.md).  The same strip
        // sums in the same integer type: bit-identical.
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(cnt[i] > (uint32_t)kSatMaxArea) != 0, 0)) {
            if (cnt[i] > (uint32_t)kSatMaxArea) {
                uint32_t sb = 0, sg = 0, sr = 0;
                const int wd = xb[i] - xa[i];
                if (wd <= kSatMaxArea) {                            // every nominal window: strips of whole rows
                    const int rh = max(kSatMaxArea / wd, 1);
                    const uint32_t cs = 8u * (uint32_t)xa[i] + 24u, ce = 8u * (uint32_t)xb[i] + 24u;
                    u64 Dp = C[i][1] - C[i][0];                     // the first corner row
                    for (int ys = ya[i] + rh; ys < yb[i]; ys += rh) {            // the rows between the strips
                        const uint32_t r1 = (uint32_t)(ys - trow0) * pitch8;
                        const u64 D1 = tab_load(rsrc, r1 + ce) - tab_load(rsrc, r1 + cs);
                        add_fields(D1 - Dp, sb, sg, sr);
                        Dp = D1;
                    }
                    add_fields((C[i][3] - C[i][2]) - Dp, sb, sg, sr);                  // the strip that ends at the last corner row
                } else {                                            // a row wider than a strip may be (depths far above 255 only): strips in columns too
                    const int cw = kSatMaxArea, rh = 1;
                    for (int xs = xa[i]; xs < xb[i]; xs += cw) {
                        const int xe = min(xs + cw, xb[i]);
                        const uint32_t cs = 8u * (uint32_t)xs + 24u, ce = 8u * (uint32_t)xe + 24u;
                        const uint32_t r0 = (uint32_t)(ya[i] - trow0) * pitch8;
                        u64 D0 = tab_load(rsrc, r0 + ce) - tab_load(rsrc, r0 + cs);
                        for (int ys = ya[i]; ys < yb[i]; ys += rh) {
                            const int ye = min(ys + rh, yb[i]);
                            const uint32_t r1 = (uint32_t)(ye - trow0) * pitch8;
                            const u64 D1 = tab_load(rsrc, r1 + ce) - tab_load(rsrc, r1 + cs);
                            add_fields(D1 - D0, sb, sg, sr);
                            D0 = D1;
                        }
                    }
                }
                res = quot3_exact_or_f32(sb, sg, sr, cnt[i]);
            }
        }
        // (a banded table) a window that reaches beyond the slice's rows -- a depth above 255: no depth map -- is summed by its wave from
        // the image, exactly (as k_defocus_tile does with windows beyond its region), and the host is told: this context's later calls
        // build the one whole-image table again (rtdd_internal.hpp defocus_band_sticky)
        {
            unsigned long long todo = __builtin_amdgcn_ballot_w64(cnt[i] != 0u && (ya[i] < trow0 || yb[i] > trow0 + trows));
            if (__builtin_expect(todo != 0, 0)) {
                const bool mine = (todo >> lane) & 1ull;
                if (lane == 0 && nonlocal_word) __hip_atomic_fetch_or(nonlocal_word, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                uint32_t sb = 0, sg = 0, sr = 0;
                while (todo) {
                    const int L = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int wya = __builtin_amdgcn_readlane(ya[i], L), wyb = __builtin_amdgcn_readlane(yb[i], L);
                    const int wxa = __builtin_amdgcn_readlane(xa[i], L), wxb = __builtin_amdgcn_readlane(xb[i], L);
                    uint32_t tb = 0, tg = 0, tr = 0;
                    for (int r = wya; r < wyb; r++) {
                        const uint8_t *row = orig + (size_t)r * op;
                        for (int c = wxa + lane; c < wxb; c += 64) { tb += row[3 * (size_t)c]; tg += row[3 * (size_t)c + 1]; tr += row[3 * (size_t)c + 2]; }
                    }
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) { tb += __shfl_xor(tb, m); tg += __shfl_xor(tg, m); tr += __shfl_xor(tr, m); }
                    if (lane == L) { sb = tb; sg = tg; sr = tr; }
                }
                if (mine) res = quot3_exact_or_f32(sb, sg, sr, cnt[i]);
            }
        }
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(cnt[i] == 0u) != 0, 0)) {   // count == 0 (src/GPUDepthEffect.cu:62-66): the pixel itself
            if (cnt[i] == 0u) res = load_bgr(orig + (size_t)yc * op + 3 * (size_t)xc);
        }
        if (y < row1) {                                             // wave-uniform (row1 <= rows: this launch's last output row + 1)
            uint8_t *arow = art + (size_t)y * ap;
            if (whole) store_bgr_quads(arow, x0, lane, res);
            else if (x < cols) store_bgr(arow + 3 * (size_t)x, res);
        }     // wave-uniform (row1 <= rows: this launch's last output row + 1)
    }
}

// ---- defocus without a global table: images up to ~1080p (kernelSize / 2 <= kDtHM) ------------------------------------------------
// The four launches above are each a load -> compute -> store round on the whole image: 5.4 + 6.3 + 11.9 + 12.2 us at 1080p, mostly
// kernel boundaries and memory round trips (the table is written and read back: 16.6 MB each way).  When the largest nominal window
// is small -- half-width hm = kernelSize / 2 <= 28, i.e. images up to a 2280-pixel diagonal: 1080p, and every pair of the bundled
// dataset -- ONE launch does it: a workgroup takes a 64 x 24 tile of output pixels, builds the summed-area table of the region its
// windows can reach ((24 + 2 hm) rows x (64 + 2 hm) columns, <= 80 x 124 packed 64-bit entries = 78 KB) in LDS and reads its four
// corners from there.  Packed fields of a LOCAL prefix overflow (the region holds more than 8224 pixels), but a window of
// <= 56 x 56 pixels never does, and the four-corner combination is exact mod 2^64 (the carries of the prefixes cancel, as above).
//   * build: the region is cut into 8 horizontal chunks, one per half-wave ("worker"): lane = four consecutive columns, the worker
//     walks its <= 10 rows top to bottom with running column sums in registers and a 32-lane prefix scan per row (every load of the
//     tile is issued before the first is used); the chunks' last rows go through LDS, each worker adds what lies above its chunk and
//     writes its rows once.
//   * lookup: as k_defocus, the corners from LDS.
//   * a pixel whose window is larger than the region allows (depth > 255, or not a depth at all) is summed by its wave directly from
//     the image, exactly and in bounded time (sums in u32: the whole image is < 2^32 / 255 pixels here); the results are what the
//     table path gives (integer sums, then the same quotient code).
// Tile height TH: 24 rows (region <= 80 rows = 78 KB: the most LDS lets two workgroups per CU have) or, for images whose 16-row tiles
// all run at once (<= 512: up to ~700 x 700), 16 rows -- there a tile's latency is the launch's, and a shorter tile is done sooner.
template <bool VEC, int kDtH, bool FOCUS>
__global__ __launch_bounds__(256, 2) void k_defocus_tile(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                         uint8_t *__restrict__ art, size_t ap, int rows, int cols, int kernelSize, int hm,
                                                         int gx, int ntiles, int xcd_tiles, int *__restrict__ nonlocal_word,
                                                         float focus, const float *__restrict__ focus_px) {
    constexpr int kDtRH = kDtH + 2 * kDtHM, kDtRowsPer = (kDtRH + kDtWorkers - 1) / kDtWorkers;
    __shared__ u64 S[kDtRH][kDtRW];                                 // the region's summed-area table, S[r - R0][c - C0]: <= 79 360 B, two workgroups per CU
    const int tile = band_tile(blockIdx.x, xcd_tiles);
    if (tile >= ntiles) return;
    // (loads and table build at a raised wave priority, the lookups at the normal one: of the two workgroups on a CU the one still
    // building gets ahead of the other's lookups -- 1080p 27.3 -> 26.5 us, 672 x 624 8.9 -> 8.5)
    __builtin_amdgcn_s_setprio(2);
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
    const int tx0 = (tile % gx) * kDtW, ty0 = (tile / gx) * kDtH;

    // ---- every load of the tile first: the region's pixels (this thread: 4 columns x <= 9 rows) and the output pixels' depth / colour ----
    const int R0 = ty0 - hm, C0 = (tx0 - hm) & ~3;                  // (a multiple of four, also when negative: groups of four never straddle column 0)
    const int rh = kDtH + 2 * hm, rpw = (rh + kDtWorkers - 1) / kDtWorkers;      // region rows, rows per worker
    const int worker = tid >> 5, wl = tid & 31, gcol = C0 + 4 * wl;
    const bool group_ok = wl < kDtRW / 4 && gcol >= 0 && gcol < cols;
    raw12 raw[kDtRowsPer];
    if (VEC && C0 >= 0 && C0 + kDtRW <= cols) {
        const int gc = wl < kDtRW / 4 ? gcol : C0;
#pragma unroll
        for (int i = 0; i < kDtRowsPer; i++) {
            const int r = R0 + worker * rpw + i, rc = min(max(r, 0), rows - 1);
            const uint32_t *q = (const uint32_t *)(orig + (size_t)rc * op + 3 * (size_t)gc);
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
            const bool ok = wl < kDtRW / 4 && i < rpw && r == rc;
            raw[i] = raw12{ok ? w0 : 0u, ok ? w1 : 0u, ok ? w2 : 0u};
        }
    } else {
#pragma unroll
        for (int i = 0; i < kDtRowsPer; i++) {
            const int r = R0 + worker * rpw + i;
            raw[i] = raw12{0, 0, 0};
            if (group_ok && i < rpw && r >= 0 && r < rows) raw[i] = load_raw<VEC>(orig + (size_t)r * op, gcol, cols);
        }
    }
    const int x = tx0 + lane, xc = min(x, cols - 1);
    const bool whole = VEC && tx0 + kDtW <= cols;                   // wave-uniform: the dword path for orig / art
    const int j = lane & 3;
    constexpr int NR = kDtH / 4;                                    // output rows per wave
    float d[NR];
    uint32_t opx[NR];
    const float f = FOCUS ? focal_depth(focus, focus_px) : 0.0f;   // (FOCUS: k_defocus; |d - f| <= 255 while both are depths: the region still holds)
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const int y = min(ty0 + wv * NR + i, rows - 1);
        d[i] = ((const float *)((const char *)depth + (size_t)y * dp))[xc];
        if (FOCUS) d[i] = fabsf(d[i] - f);
        const uint8_t *orow = orig + (size_t)y * op;
        if (whole) {
            const uint32_t L = j < 3 ? ((const uint32_t *)(orow + 3 * (size_t)tx0))[3 * (lane >> 2) + j] : 0u;
            const uint32_t prv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)L, 0x90, 0xF, 0xF, true);   // quad_perm:[0,0,1,2]
            opx[i] = __builtin_amdgcn_alignbit(L, prv, (32 - 8 * j) & 31) & 0xFFFFFFu;
        } else {
            opx[i] = load_bgr(orow + 3 * (size_t)xc);
        }
    }

    // ---- the chunk's rows: running column sums, row prefix; kept in registers until the chunks above are known ----
    u64 col[4] = {0, 0, 0, 0}, v[kDtRowsPer][4];
#pragma unroll
    for (int i = 0; i < kDtRowsPer; i++) {
        u64 px[4];
        unpack4(raw[i].w0, raw[i].w1, raw[i].w2, px);          // (zeros where nothing was loaded: outside the image or the region)
#pragma unroll
        for (int k = 0; k < 4; k++) col[k] += px[k];
        const u64 s0 = col[0], s1 = s0 + col[1], s2 = s1 + col[2], s3 = s2 + col[3];
        const u64 excl = half_incl_scan64(s3) - s3;
        v[i][0] = s0 + excl; v[i][1] = s1 + excl; v[i][2] = s2 + excl; v[i][3] = s3 + excl;
    }
    // each chunk's last row (its column totals, row-prefixed) goes through the table's own row `worker` -- LDS has no room for a
    // second array -- and is read back by the chunks below before any final row is written
    if (wl < kDtRW / 4) {
        u64x2 *q = (u64x2 *)&S[worker][4 * wl];
        q[0] = u64x2{v[kDtRowsPer - 1][0], v[kDtRowsPer - 1][1]}; q[1] = u64x2{v[kDtRowsPer - 1][2], v[kDtRowsPer - 1][3]};
    }
    __syncthreads();
    u64 base[4] = {0, 0, 0, 0};
    if (wl < kDtRW / 4) {
        for (int k = 0; k < worker; k++) {
            const u64x2 *q = (const u64x2 *)&S[k][4 * wl];
            const u64x2 a = q[0], b = q[1];
            base[0] += a.a; base[1] += a.b; base[2] += b.a; base[3] += b.b;
        }
    }
    __syncthreads();
    if (wl < kDtRW / 4) {
#pragma unroll
        for (int i = 0; i < kDtRowsPer; i++) {
            const int rr = worker * rpw + i;
            if (i < rpw && rr < rh) {
                u64x2 *q = (u64x2 *)&S[rr][4 * wl];
                q[0] = u64x2{v[i][0] + base[0], v[i][1] + base[1]}; q[1] = u64x2{v[i][2] + base[2], v[i][3] + base[3]};
            }
        }
    }
    __syncthreads();

    __builtin_amdgcn_s_setprio(0);
    // ---- lookups (k_defocus with the corners in LDS) ----
    // The common case -- the window lies inside the region -- is straight-line code for the whole wave: clamped LDS addresses, selects
    // instead of branches, the quotients by quot3_u8 (count <= 56 x 56); what it computes for a lane whose window does not
    // fit is discarded.  Such lanes (a depth above 255 * (2 hm + 1) / kernelSize, never a depth map's) are summed from the image by
    // their wave under ONE wave-uniform branch per row of output.
    const int rh1 = rh - 1;
    bool have_whole = false;                                        // this wave has summed the WHOLE image once (what an infinite or garbage depth asks for)
    uint32_t whole_b = 0, whole_g = 0, whole_r = 0;
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const int y = ty0 + wv * NR + i, yc = min(y, rows - 1);
        const int h = half_window(kernelSize, d[i]);                // <= 2^21: the sums below stay in int
        const int ya = max(yc - h, 0), yb = min(yc + h, rows);
        const int xa = max(xc - h, 0), xb = min(xc + h, cols);
        const int wd = xb - xa, ht = yb - ya;
        const bool has = wd > 0 && ht > 0, local = h <= hm;
        // T(r, c) of the region's table at the four corners; a row / column before the region sums to nothing
        const int r1 = min(max(yb - 1 - R0, 0), rh1), r0 = min(ya - 1 - R0, rh1), c1 = min(max(xb - 1 - C0, 0), kDtRW - 1), c0 = min(xa - 1 - C0, kDtRW - 1);
        const int r0c = max(r0, 0), c0c = max(c0, 0);
        const u64 t11 = S[r1][c1], t10 = S[r1][c0c], t01 = S[r0c][c1], t00 = S[r0c][c0c];
        const u64 X = t11 - (c0 < 0 ? 0ull : t10) - (r0 < 0 ? 0ull : t01) + ((r0 < 0 || c0 < 0) ? 0ull : t00);
        const uint32_t fb = (uint32_t)(X & kSatFieldMask), fg = (uint32_t)((X >> 21) & kSatFieldMask), fr = (uint32_t)(X >> 42);
        const uint32_t cnt = (uint32_t)__mul24(ht, wd);             // (exact for a window inside the region; recomputed below otherwise)
        const uint32_t fast = quot3_u8(fb, fg, fr, cnt, __builtin_amdgcn_rcpf((float)cnt));   // (an empty window: discarded below)
        uint32_t res = (has && local) ? fast : opx[i];              // count == 0 (:62-66): the pixel itself
        unsigned long long todo = __builtin_amdgcn_ballot_w64(has && !local);
        if (__builtin_expect(todo != 0, 0)) {                       // windows beyond the region: the wave sums them from the image, one pixel at a time
            // (the host hears of it at its next synchronisation and sends this context's later calls to the table: rtdd_internal.hpp
            // defocus_table_sticky -- a window costs its area here, the table a constant)
            if (lane == 0) __hip_atomic_fetch_or(nonlocal_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t sb = 0, sg = 0, sr = 0;
            while (todo) {
                const int L = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int wya = __builtin_amdgcn_readlane(ya, L), wyb = __builtin_amdgcn_readlane(yb, L);
                const int wxa = __builtin_amdgcn_readlane(xa, L), wxb = __builtin_amdgcn_readlane(xb, L);
                const bool whole_image = wya == 0 && wxa == 0 && wyb == rows && wxb == cols;
                uint32_t tb = whole_b, tg = whole_g, tr = whole_r;
                if (!(whole_image && have_whole)) {
                    tb = tg = tr = 0;
                    for (int r = wya; r < wyb; r++) {
                        const uint8_t *row = orig + (size_t)r * op;
                        for (int c = wxa + lane; c < wxb; c += 64) { tb += row[3 * (size_t)c]; tg += row[3 * (size_t)c + 1]; tr += row[3 * (size_t)c + 2]; }
                    }
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) { tb += __shfl_xor(tb, m); tg += __shfl_xor(tg, m); tr += __shfl_xor(tr, m); }
                    if (whole_image) { have_whole = true; whole_b = tb; whole_g = tg; whole_r = tr; }
                }
                if (lane == L) { sb = tb; sg = tg; sr = tr; }
            }
            if (has && !local) res = quot3_exact_or_f32(sb, sg, sr, (uint32_t)ht * (uint32_t)wd);
        }
        if (y < rows) {                                             // wave-uniform
            uint8_t *arow = art + (size_t)y * ap;
            if (whole) store_bgr_quads(arow, tx0, lane, res);
            else if (x < cols) store_bgr(arow + 3 * (size_t)x, res);
        }    // wave-uniform
    }
}

static inline dim3 grid64x4(int rows, int cols) { return dim3((cols + 63) / 64, (rows + 3) / 4); }

template <int MODE>
static int launch_blend(rtdd_ctx *ctx, const uint8_t *orig, size_t op, const uint8_t *gray, size_t gp, const float *depth, size_t dp,
                        uint8_t *art, size_t ap, int rows, int cols, float beta = 2.0f, uint32_t air = 0xFFFFFFu) {
    const bool aligned = rows_aligned(orig, op) && rows_aligned(art, ap) && rows_aligned(depth, dp, 16) && (MODE != 0 || rows_aligned(gray, gp));
    const dim3 grid = aligned ? dim3((cols + 255) / 256, (rows + 3) / 4) : grid64x4(rows, cols);
#define RTDD_BL_LAUNCH(C, V) hipLaunchKernelGGL((k_blend<MODE, C, V>), grid, dim3(256), 0, ctx->stream, orig, op, gray, gp, depth, dp, art, ap, rows, cols, beta, air)
    if (ctx->opt.fp_contract != 0) { if (aligned) RTDD_BL_LAUNCH(true, true); else RTDD_BL_LAUNCH(true, false); }
    else { if (aligned) RTDD_BL_LAUNCH(false, true); else RTDD_BL_LAUNCH(false, false); }
#undef RTDD_BL_LAUNCH
    RTDD_LAUNCH_CHECK(ctx, "k_blend");
    return RTDD_OK;
}

// The body of rtdd_simulate_defocus (FOCUS false) and rtdd_simulate_refocus (FOCUS true: the kernels size each window by
// |depth - f|, f = *focus_px or `focus`).  kernelSize <= 255 for a refocus (effects_api.cpp): every window of a depth map stays within the
// domains the packed fields and the quotients are proven on, and the reach kernelSize / 2 that the tile region and the slices are sized
// for still bounds it (|d - f| <= 255 while both lie in [0, 255]; anything else takes the same fall-backs as an out-of-range depth).
template <bool FOCUS>
static int defocus_body(rtdd_ctx *ctx, const uint8_t *orig, size_t op, const float *depth, size_t dp, uint8_t *art, size_t ap, int rows, int cols,
                        int kernelSize, float focus, const float *focus_px) {
    // small nominal windows (up to ~1080p): one launch, per-tile tables in LDS (k_defocus_tile).  RTDD_OPT_DEFOCUS_PATH: 0 automatic, 1 the
    // global table always, 2 the tile kernel wherever its region fits.
    if (ctx->opt.defocus_path != 1 && !(ctx->opt.defocus_path == 0 && ctx->defocus_table_sticky) && kernelSize / 2 <= kDtHM && (size_t)rows * cols < (1ull << 32) / 255) {
        const DtGrid t = dt_grid(ctx, rows, cols);
#define RTDD_DT_LAUNCH(V, H) hipLaunchKernelGGL((k_defocus_tile<V, H, FOCUS>), t.grid, dim3(256), 0, ctx->stream, orig, op, depth, dp, art, ap, rows, cols, kernelSize, kernelSize / 2, t.gx, t.ntiles, t.xcd_tiles, ctx->sync_words + kSyncNonLocal, focus, focus_px)
        if (rows_aligned(orig, op) && rows_aligned(art, ap)) { if (t.low) RTDD_DT_LAUNCH(true, 16); else RTDD_DT_LAUNCH(true, 24); }
        else { if (t.low) RTDD_DT_LAUNCH(false, 16); else RTDD_DT_LAUNCH(false, 24); }
#undef RTDD_DT_LAUNCH
        RTDD_LAUNCH_CHECK(ctx, "k_defocus_tile");
        ctx->defocus_last_path = 2;
        note_status_writer(ctx);                     // (kSyncNonLocal: the next synchronising call reads the control words, check_persistent_status)
        return RTDD_OK;
    }
    const int tp = (cols + 3) / 4 * 4;                                  // entries the build writes per row: 32-byte aligned groups of four
    // the table is padded -- one zero row above, four zero entries left of every row (k_defocus): T'[r + 1][c + 4] = T(r, c)
    const int tpitch = tp + 4;
    // Round 6, BANDED tables (RTDD_OPT_DEFOCUS_SLICE_MB > 0; OFF by default: measured, it does not pay -- see the end of this comment).  A whole-image table is 8 bytes per pixel: 66 MB at 4K, 265 MB at 8K -- more than the 256 MiB Infinity
    // Cache, so every corner of an 8K lookup was a gather from HBM (729 us smooth, 2.9 ms with a random depth per pixel).  Rectangle sums
    // are differences, so a table with its origin at any row above the window serves: the image is cut into horizontal slices of output
    // rows, each slice builds the table of ITS rows plus the tallest nominal window's reach (kernelSize / 2 rows above and below: a
    // depth map is <= 255) -- into the same buffer, which therefore stays in the Infinity Cache -- and looks its pixels up in it.  A
    // window that reaches further (a depth above 255) is summed from the image by its wave and reported (k_defocus); the context then
    // goes back to one whole-image table (defocus_band_sticky).  Same integer sums, same quotients: bit-identical.
    // MEASURED (profiles/r06_defocus_slices.txt, one call): 8K smooth 725 us as one table, 762 in 5 slices of 64 MB, 955 in 14 of 32 MB;
    // with a real depth map 520 / 634 / 785; random depth 2905 / 2976 / 3064.  What made 8K 9 x 4K's time for 4 x the pixels was not the
    // table leaving the Infinity Cache but its LINES leaving the XCD's L2 between a window's bottom- and top-edge reads (2 h rows x the
    // whole image width = 13.5 MB at 8K): the lookup's column strips per XCD (k_defocus strip_w, below) are what pays -- 8K 727 -> 620 us
    // smooth, 522 -> 399 with a real depth map, 2888 -> 1342 random.  The slices stay as an option: they are what lets an image whose
    // whole table would pass 4 GiB (rows x cols > 2^29) be processed at all.
    const int reach = kernelSize / 2;
    const size_t slice_budget = (size_t)ctx->opt.defocus_slice_mb << 20;          // RTDD_OPT_DEFOCUS_SLICE_MB (default 0: never band)
    const size_t row_bytes = (size_t)tpitch * sizeof(u64);
    int slice_rows = rows;                                              // output rows per slice
    const bool want_bands = slice_budget > 0 && !ctx->defocus_band_sticky && ctx->opt.defocus_path != 1 &&
                            ((size_t)rows + 1) * row_bytes > 2 * slice_budget;       // (a table that fits the cache twice over is left whole: 4K)
    if (want_bands) {
        const long fit = (long)(slice_budget / row_bytes) - 2L * reach - 1;
        slice_rows = fit >= 64 ? (int)fit : 64;
        slice_rows = slice_rows / 8 * 8;                                // whole lookup tiles (8 rows)
        if (slice_rows >= rows) slice_rows = rows;
    }
    const int nslices = (rows + slice_rows - 1) / slice_rows;
    const int trows_max = nslices == 1 ? rows : (slice_rows + 2 * reach < rows ? slice_rows + 2 * reach : rows);
    // band height: one workgroup per band builds the table, so enough bands to occupy the chip (270 / 135 / 135 workgroups of 8 / 16 / 16
    // waves at 1080p / 4K / 8K); a band costs 8 B per column three times over (colsum, its scan, the build's read)
    const int RB = trows_max <= 1536 ? 4 : trows_max <= 3072 ? 16 : 32;
    const int nbands_max = (trows_max + RB - 1) / RB;
    const size_t table_entries = ((size_t)trows_max + 1) * tpitch;
    // k_defocus addresses the padded table with 32-bit BYTE offsets (one 24-bit multiply per corner row) through a buffer resource whose
    // num_records is a 32-bit byte count: the table must stay below 4 GiB and both factors of that multiply below 2^24.  check_effect
    // only bounds rows^2 + cols^2 < 2^31, which admits rows x cols up to 2^30 -- an 8.6 GB table whose offsets would wrap and read zeros.
    if (table_entries * sizeof(u64) >= (1ull << 32) || (size_t)tpitch * sizeof(u64) >= (1u << 24) || (size_t)trows_max + 1 >= (1u << 24))
        return fail(ctx, RTDD_ERR_INVALID, "image too large for the defocus table (its 8 bytes per pixel must stay below 4 GiB: about 536 million pixels)");
    const size_t need = ((table_entries + (size_t)nbands_max * tp) * sizeof(u64) + 256) / sizeof(uint32_t);   // padded table + band bases, in u32 words
    if (const int st = ensure_sat(ctx, need)) return st;
    u64 *Tpad = (u64 *)ctx->sat, *T = Tpad + tpitch + 4, *base = Tpad + table_entries;
    if (ctx->sat_rows != trows_max || ctx->sat_cols != cols) {          // another geometry: the padding lies elsewhere -- zero the table once (the build never writes the padding)
        RTDD_HIP(ctx, hipMemsetAsync(Tpad, 0, table_entries * sizeof(u64), ctx->stream));
        ctx->sat_rows = trows_max; ctx->sat_cols = cols;
    }
    const bool vin = rows_aligned(orig, op), vout = vin && rows_aligned(art, ap);
    for (int sl = 0; sl < nslices; sl++) {
        const int row0 = sl * slice_rows, row1 = row0 + slice_rows < rows ? row0 + slice_rows : rows;
        const int trow0 = nslices == 1 ? 0 : (row0 - reach > 0 ? row0 - reach : 0);
        const int trow1 = nslices == 1 ? rows : (row1 + reach < rows ? row1 + reach : rows);
        const int trows = trow1 - trow0, nbands = (trows + RB - 1) / RB;
        const uint8_t *o_sl = orig + (size_t)trow0 * op;               // the slice's rows of the image: the table's origin is its first row
        const dim3 g1((tp / 4 + 255) / 256, nbands);
        if (vin) hipLaunchKernelGGL(k_sat_colsum<true>, g1, dim3(256), 0, ctx->stream, o_sl, op, base, tp, trows, cols, RB);
        else hipLaunchKernelGGL(k_sat_colsum<false>, g1, dim3(256), 0, ctx->stream, o_sl, op, base, tp, trows, cols, RB);
        RTDD_LAUNCH_CHECK(ctx, "k_sat_colsum");
        int scan_waves = (nbands + 3) / 4; if (scan_waves > 16) scan_waves = 16;
        hipLaunchKernelGGL(k_sat_colbase, dim3((tp + 63) / 64), dim3(64 * scan_waves), 0, ctx->stream, base, tp, nbands);
        RTDD_LAUNCH_CHECK(ctx, "k_sat_colbase");
        int build_waves = (tp / 4 + 63) / 64; if (build_waves > 16) build_waves = 16;
        if (vin) hipLaunchKernelGGL(k_sat_build<true>, dim3(nbands), dim3(64 * build_waves), 0, ctx->stream, o_sl, op, base, T, tp, trows, cols, RB, tpitch);
        else hipLaunchKernelGGL(k_sat_build<false>, dim3(nbands), dim3(64 * build_waves), 0, ctx->stream, o_sl, op, base, T, tp, trows, cols, RB, tpitch);
        RTDD_LAUNCH_CHECK(ctx, "k_sat_build");
        const LookupGrid t = lookup_grid(ctx, row1 - row0, cols, 4 * kLk2Rows, reach, row_bytes);
        int *nlw = nslices > 1 ? ctx->sync_words + kSyncNonLocal : nullptr;
        if (vout) hipLaunchKernelGGL((k_defocus<true, FOCUS>), t.grid, dim3(256), 0, ctx->stream, orig, op, depth, dp, Tpad, tpitch, art, ap, rows, cols, kernelSize, t.gx, t.ntiles, t.xcd_tiles, row0, row1, trow0, trows, nlw, t.strip_w, focus, focus_px);
        else hipLaunchKernelGGL((k_defocus<false, FOCUS>), t.grid, dim3(256), 0, ctx->stream, orig, op, depth, dp, Tpad, tpitch, art, ap, rows, cols, kernelSize, t.gx, t.ntiles, t.xcd_tiles, row0, row1, trow0, trows, nlw, t.strip_w, focus, focus_px);
    }
    if (nslices > 1) note_status_writer(ctx);                           // (kSyncNonLocal: a window beyond a slice -> the whole-image table from the next synchronisation on)
    RTDD_LAUNCH_CHECK(ctx, "k_defocus");
    ctx->defocus_last_path = 1;
    ctx->defocus_last_slices = nslices;
    return RTDD_OK;
}

// Every depth effect (arguments checked by effects_api.cpp or live.cpp): k_blend's three modes and the two defocus bodies.
int launch_effect(rtdd_ctx *ctx, const Effect &e) {
    switch (e.kind) {
        case RTDD_EFFECT_DEFOCUS:
            return defocus_body<false>(ctx, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols,
                                       window_scale(0.025, e.rows, e.cols), 0.0f, nullptr);     // :42, evaluated once on the host
        case Effect::kRefocus:
            return defocus_body<true>(ctx, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols,
                                      e.kernelSize, e.focusDepth, pixel_ptr(e.depth, e.depthPitch, e.focusX, e.focusY));
        case Effect::kLensBlur: return launch_lens_blur(ctx, e);       // lens_blur.hip
        case Effect::kRelight: return launch_relight(ctx, e);          // relight.hip
        case Effect::kRelightShadow: return launch_relight_shadow(ctx, e);     // relight_shadow.hip
        case Effect::kParallax:
        case Effect::kParallaxLayered: return launch_parallax(ctx, e); // parallax.hip
        case Effect::kAmbientOcclusion: return launch_ambient_occlusion(ctx, e);   // ambient_occlusion.hip
        case Effect::kLighting: return launch_lighting(ctx, e);        // lighting.hip
        case Effect::kBokeh: return launch_bokeh(ctx, e);              // bokeh.hip
        case Effect::kComposite: return launch_composite(ctx, e);      // composite.hip
        case Effect::kRemove: return launch_remove(ctx, e);            // remove.hip
        case Effect::kLift:
        case Effect::kLiftMatte: return launch_lift(ctx, e);           // remove.hip
        case Effect::kMaskDistance:
        case Effect::kRefineMask: return launch_mask_distance(ctx, e); // mask_distance.hip
        case RTDD_EFFECT_DESATURATION:
            return launch_blend<0>(ctx, e.original, e.originalPitch, e.gray, e.grayPitch, e.depth, e.depthPitch, e.artistic, e.artisticPitch,
                                   e.rows, e.cols);
        case RTDD_EFFECT_HAZE:
            return launch_blend<1>(ctx, e.original, e.originalPitch, nullptr, 0, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols);
        case Effect::kHazeEx:
            return launch_blend<2>(ctx, e.original, e.originalPitch, nullptr, 0, e.depth, e.depthPitch, e.artistic, e.artisticPitch, e.rows, e.cols,
                                   e.beta, e.air);
        case Effect::kStereo: {
            const float *zp = pixel_ptr(e.depth, e.depthPitch, e.zeroX, e.zeroY);      // the pixel form of z0
            const dim3 g((e.cols + kStW - 1) / kStW, e.rows);
            if (rows_aligned(e.original, e.originalPitch) && rows_aligned(e.artistic, e.artisticPitch))
                hipLaunchKernelGGL(k_stereo<true>, g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic,
                                   e.artisticPitch, e.rows, e.cols, e.disparity, e.zeroDepth, zp, e.stereoMode);
            else hipLaunchKernelGGL(k_stereo<false>, g, dim3(256), 0, ctx->stream, e.original, e.originalPitch, e.depth, e.depthPitch, e.artistic,
                                    e.artisticPitch, e.rows, e.cols, e.disparity, e.zeroDepth, zp, e.stereoMode);
            RTDD_LAUNCH_CHECK(ctx, "k_stereo");
            return RTDD_OK;
        }
        default: return fail(ctx, RTDD_ERR_INVALID, "unknown depth effect");
    }
}

}  // namespace rtdd
