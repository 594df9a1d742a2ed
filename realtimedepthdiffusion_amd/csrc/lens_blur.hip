// lens_blur.hip -- rtdd_simulate_lens_blur with RTDD_APERTURE_DISC: refocus with a round aperture (include/rtdd.h, DESIGN.md section 4
// "Lens blur").  No reference behaviour: the definition is the header's, restated three times over in tests/lens_blur_ref.py.
//
// Per pixel (x, y): k = clamp((int)(K |d - f| / 255.0), 0, 255) as refocus sizes its box; the window is the pixels (px, py) of the image with
// 4 ((px - x)^2 + (py - y)^2) <= k^2 -- rows dy = -h .. h, h = k / 2, and in row dy the span x - w .. x + w, w = isqrt(k^2 / 4 - dy^2)
// (integer division: 4 dy^2 is a multiple of four) -- and the result (uchar)(sum / count) per channel.  The centre always belongs, so
// count >= 1; k <= 1 is the pixel itself.  A disc of k = 255 holds 51 101 pixels (< 2^16) and its channel sums are < 2^24: f32 sums in
// any order are exact, and so are the integer sums and the quotients of quot3_u8 used here.
//
// A disc is no difference of four corners: it is one span per window row, 2 h + 1 spans, each the difference of two entries of a table
// of ROW prefixes E[r][i] = packed sum of the pixels of row r left of column i (the 3 x 21-bit packing of the defocus table,
// effect_common.hpp).  A span is <= 255 pixels, so its packed difference is exact mod 2^64 whatever the prefixes have carried into each
// other; a sum of spans stays exact while they hold <= kSatMaxArea pixels -- a whole disc up to k = 102, 32 rows of any disc.
//   k_lens_tile       K / 2 <= kDtHM: one launch; a workgroup builds the row prefixes of the region its 64 x 24 (64 x 16) tile's discs can
//                     reach in LDS and every pixel walks its rows there.
//   k_lens_rowprefix  otherwise: the row prefixes of the whole image in global memory (the context's defocus table buffer) ...
//   k_lens_gather     ... and the same walk through L2.
#include "rtdd_internal.hpp"
#include "effect_common.hpp"

namespace rtdd {

// k of the header: (int)((double)((float)K * dist) / 255.0) clamped to [0, 255], 0 for a NaN.  v = (float)K * dist is an f32, so the
// double quotient never rounds across an integer (half_window's argument, effect_kernels.hip) and (int) of it is floor(v / 255):
// q = (int)(v / 255) in f32 is within one of it, the remainder v - 255 q is exact, one correction step.  v >= 255 * 255 gives 255.
__device__ __forceinline__ int disc_diameter(int kernelSize, float dist) {
    const float v = __builtin_amdgcn_fmed3f((float)kernelSize * dist, 0.0f, 65025.0f);      // (a NaN gives 0)
    int k = (int)(v * (1.0f / 255.0f));
    const float r = __builtin_fmaf(-255.0f, (float)k, v);           // exact
    k += r < 0.0f ? -1 : (r >= 255.0f ? 1 : 0);
    return k;                                                       // 0 .. 255
}

// isqrt(n) for 0 <= n <= 16256 (255^2 / 4): v_sqrt_f32 is within one ulp (2^-17 at 127), sqrt(m^2 + 0.5) lies at least 0.25 / 127 above m
// and sqrt(m^2 - 0.5) as far below it -- the truncation cannot land on the wrong side.
__device__ __forceinline__ int disc_isqrt(int n) { return (int)__builtin_amdgcn_sqrtf((float)n + 0.5f); }

// The columns of row dy of the disc q4 = k^2 / 4 around x, clipped to the image: [xa, xb1).  Empty (xa == xb1) for a row beyond the
// disc, q4 < dy^2 -- a lane that has finished while its wave walks on.
__device__ __forceinline__ void disc_span(int q4, int dy, int x, int cols, int &xa, int &xb1) {
    const int n = q4 - dy * dy, w = disc_isqrt(max(n, 0));
    xa = max(x - w, 0);
    xb1 = n >= 0 ? min(x + w + 1, cols) : xa;
}

__device__ __forceinline__ uint32_t disc_quot(u64 X, uint32_t sb, uint32_t sg, uint32_t sr, uint32_t cnt) {
    add_fields(X, sb, sg, sr);
    return quot3_u8(sb, sg, sr, cnt, __builtin_amdgcn_rcpf((float)cnt));
}

// a wave's 64 results b | g << 8 | r << 16 of row y, columns x0 .. x0 + 63, to the image.  whole (wave-uniform: 4-byte aligned rows and
// all 64 columns inside the image): `art` moves as dwords (store_bgr_quads); else bytes, column by column
__device__ __forceinline__ void store_row(uint8_t *__restrict__ art, size_t ap, int y, int x0, int lane, int cols, bool whole, uint32_t res) {
    uint8_t *arow = art + (size_t)y * ap;
    const int x = x0 + lane;
    if (whole) store_bgr_quads(arow, x0, lane, res);
    else if (x < cols) store_bgr(arow + 3 * (size_t)x, res);
}

// ---- the row-prefix table in global memory ---------------------------------------------------------------------------------------
// E[r][i], i = 0 .. cols (tpitch entries per row, a multiple of four): the packed sum of row r's pixels left of column i.  One
// workgroup per row, four pixels per thread, a 64-bit DPP wave scan and one exchange of wave totals per pass over <= 4096 columns
// (k_sat_build's row step).  Every entry a lookup reads is written here -- the table depends on no padding.
template <bool VEC>
__global__ __launch_bounds__(1024) void k_lens_rowprefix(const uint8_t *__restrict__ orig, size_t op, u64 *__restrict__ E, int tpitch, int cols) {
    __shared__ u64 wtot[2][16];
    const int tid = threadIdx.x, lane = tid & 63, nt = (int)blockDim.x, nw = nt >> 6, w = wave_id();
    const uint8_t *row = orig + (size_t)blockIdx.x * op;
    u64 *erow = E + (size_t)blockIdx.x * tpitch;
    u64 carry = 0;
    int buf = 0;
    for (int x0 = 0; x0 < tpitch; x0 += nt * 4, buf ^= 1) {
        const int x = x0 + tid * 4;
        const raw12 v = load_raw<VEC>(row, x, cols);               // (zeros beyond the row's end)
        u64 px[4];
        unpack4(v.w0, v.w1, v.w2, px);
        const u64 s0 = px[0], s1 = s0 + px[1], s2 = s1 + px[2], s3 = s2 + px[3];
        const u64 incl = wave_incl_scan64(s3);
        if (lane == 63) wtot[buf][w] = incl;
        __syncthreads();                                            // (the other buffer is written again only behind the next barrier)
        const u64 t = (lane & 15) < nw ? wtot[buf][lane & 15] : 0;
        const u64 inc = row16_incl_scan64(t);
        const u64 left = carry + readlane64(inc - t, w) + (incl - s3);
        if (x < tpitch) {
            u64x2 *q = (u64x2 *)(erow + x);
            q[0] = u64x2{left, left + s0}; q[1] = u64x2{left + s1, left + s2};
        }
        carry += readlane64(inc, nw - 1);
    }
}

// The lookup: lane = pixel, wave = 64 pixels of one row, workgroup = 64 x 4 pixels; workgroup p runs on XCD p % 8 and the tiles are dealt
// by tile_of_workgroup -- a band of tile rows per XCD, or (strip_w > 0: wide images) a column strip per XCD walked row by row, so that
// the table rows a tile reads are still in that XCD's L2 from the tile above.  A wave's row is uniform: the two table rows of a step
// are scalar addresses and lanes with equal k read adjacent entries.  The loop runs to the largest h of the wave; a lane beyond its
// own disc adds empty spans.  Packed sums are unpacked every 32 rows (<= 32 x 255 pixels <= kSatMaxArea).
template <bool VEC>
__global__ __launch_bounds__(256) void k_lens_gather(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                      const u64 *__restrict__ E, int tpitch, uint8_t *__restrict__ art, size_t ap,
                                                      int rows, int cols, int kernelSize, int gx, int ntiles, int xcd_tiles, int strip_w,
                                                      float focus, const float *__restrict__ focus_px) {
    int tx, ty;
    if (!tile_of_workgroup(blockIdx.x, gx, ntiles, xcd_tiles, strip_w, tx, ty)) return;
    const int lane = threadIdx.x & 63, x0 = tx * 64, y = ty * 4 + wave_id();
    if (y >= rows) return;                                          // wave-uniform
    const int x = x0 + lane, xc = min(x, cols - 1);
    const float f = focal_depth(focus, focus_px);
    const float d = ((const float *)((const char *)depth + (size_t)y * dp))[xc];
    const int k = disc_diameter(kernelSize, fabsf(d - f)), h = k >> 1, q4 = (k * k) >> 2;
    int hw = h;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) hw = max(hw, __shfl_xor(hw, m));
    hw = __builtin_amdgcn_readfirstlane(hw);

    const u64 *e0 = E + (size_t)y * tpitch;
    int xa, xb1;
    disc_span(q4, 0, xc, cols, xa, xb1);
    u64 X = e0[xb1] - e0[xa];
    uint32_t cnt = (uint32_t)(xb1 - xa), sb = 0, sg = 0, sr = 0;
#pragma unroll 2
    for (int dy = 1; dy <= hw; dy++) {
        disc_span(q4, dy, xc, cols, xa, xb1);
        const int n = xb1 - xa;
        if (y - dy >= 0) {                                          // wave-uniform, as the next
            const u64 *e = E + (size_t)(y - dy) * tpitch;
            X += e[xb1] - e[xa]; cnt += (uint32_t)n;
        }
        if (y + dy < rows) {
            const u64 *e = E + (size_t)(y + dy) * tpitch;
            X += e[xb1] - e[xa]; cnt += (uint32_t)n;
        }
        if ((dy & 15) == 15) {                                      // 31 rows, then 32 at a time
            add_fields(X, sb, sg, sr);
            X = 0;
        }
    }
    store_row(art, ap, y, x0, lane, cols, VEC && x0 + 64 <= cols, disc_quot(X, sb, sg, sr, cnt));
}

// ---- without a global table: K / 2 <= kDtHM --------------------------------------------------------------------------------------
// k_defocus_tile's tile, region and load pattern (effect_kernels.hip) with ROW prefixes in LDS: S[r - R0][i] = packed sum of the
// pixels of row r in columns [C0, C0 + i).  The disc is symmetric -- rows y - h .. y + h, columns x - w .. x + w, inclusive -- where the
// box is half-open, and its spans need the exclusive prefix at their left end and the inclusive one at their right: kDtH + 2 hm rows and
// entries 0 .. 64 + 2 hm + 3 (the alignment of C0), 124 = kDtRW at hm = kDtHM.  Rows need nothing from each other, so the build is
// one pass and one barrier: a half-wave per chunk of rows, lane = four columns, a 32-lane scan per row.
// Lookup: a wave takes NR rows of output one after the other; LDS rows are wave-uniform, a lane's two reads per table row are 8-byte
// reads at x -+ w, adjacent lanes adjacent entries when their k agree.  k <= 57 here: the whole disc fits the packed fields.
// A disc beyond the region (h > hm: |d - f| > 255, no depth map's) is summed from the image by its wave, span by span, in u32 -- exact, at
// most 51 101 pixels -- and nothing is recorded anywhere: the disc has no fall-back path and sets no sticky flag.
template <bool VEC, int kDtH>
__global__ __launch_bounds__(256, 2) void k_lens_tile(const uint8_t *__restrict__ orig, size_t op, const float *__restrict__ depth, size_t dp,
                                                      uint8_t *__restrict__ art, size_t ap, int rows, int cols, int kernelSize, int hm,
                                                      int gx, int ntiles, int xcd_tiles, float focus, const float *__restrict__ focus_px) {
    constexpr int kDtRH = kDtH + 2 * kDtHM, kDtRowsPer = (kDtRH + kDtWorkers - 1) / kDtWorkers;
    __shared__ u64 S[kDtRH][kDtRW];                                 // <= 79 360 B: two workgroups per CU
    const int tile = band_tile(blockIdx.x, xcd_tiles);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
    const int tx0 = (tile % gx) * kDtW, ty0 = (tile / gx) * kDtH;

    // ---- every load first: the region's pixels (this thread: 4 columns x <= 10 rows), then the output pixels' depth ----
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
    constexpr int NR = kDtH / 4;                                    // output rows per wave
    const float f = focal_depth(focus, focus_px);
    int k[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const int y = min(ty0 + wv * NR + i, rows - 1);
        k[i] = disc_diameter(kernelSize, fabsf(((const float *)((const char *)depth + (size_t)y * dp))[xc] - f));
    }

    // ---- the region's row prefixes ----
    if (wl < kDtRW / 4) {
#pragma unroll
        for (int i = 0; i < kDtRowsPer; i++) {
            const int rr = worker * rpw + i;
            u64 px[4];
            unpack4(raw[i].w0, raw[i].w1, raw[i].w2, px);          // (zeros where nothing was loaded: outside the image or the region)
            const u64 s0 = px[0], s1 = s0 + px[1], s2 = s1 + px[2], s3 = s2 + px[3];
            const u64 left = half_incl_scan64(s3) - s3;
            if (i < rpw && rr < rh) {
                u64x2 *q = (u64x2 *)&S[rr][4 * wl];
                q[0] = u64x2{left, left + s0}; q[1] = u64x2{left + s1, left + s2};
            }
        }
    }
    __syncthreads();

    // ---- lookups ----
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const int y = ty0 + wv * NR + i;
        if (y >= rows) break;                                       // wave-uniform
        const int h = k[i] >> 1, q4 = (k[i] * k[i]) >> 2;
        const bool local = h <= hm;
        int hw = local ? h : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) hw = max(hw, __shfl_xor(hw, m));
        hw = __builtin_amdgcn_readfirstlane(hw);
        const int ql = local ? q4 : 0;                              // (a disc beyond the region: the pixel itself here, replaced below)
        const int xr = xc - C0, cr = cols - C0, cl = max(-C0, 0);   // the lane's column, the image's end and start, in region entries
        const int yr = y - R0;
        auto span = [&](int dy, int &a, int &b1) {
            const int n = ql - dy * dy, w = disc_isqrt(max(n, 0));
            a = max(xr - w, cl);
            b1 = n >= 0 ? min(xr + w + 1, cr) : a;
        };
        int a, b1;
        span(0, a, b1);
        u64 X = S[yr][b1] - S[yr][a];
        uint32_t cnt = (uint32_t)(b1 - a);
#pragma unroll 2
        for (int dy = 1; dy <= hw; dy++) {                          // (hw <= hm: rows yr -+ dy lie inside the region)
            span(dy, a, b1);
            const u64 up = S[yr - dy][b1] - S[yr - dy][a], dn = S[yr + dy][b1] - S[yr + dy][a];
            const uint32_t n = (uint32_t)(b1 - a);
            if (y - dy >= 0) { X += up; cnt += n; }                 // wave-uniform, as the next
            if (y + dy < rows) { X += dn; cnt += n; }
        }
        uint32_t res = disc_quot(X, 0, 0, 0, cnt);
        unsigned long long todo = __builtin_amdgcn_ballot_w64(!local);
        if (__builtin_expect(todo != 0, 0)) {                       // discs beyond the region: the wave sums them from the image, one at a time
            uint32_t sb = 0, sg = 0, sr = 0, sn = 0;
            while (todo) {
                const int L = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int wx = __builtin_amdgcn_readlane(xc, L), wk = __builtin_amdgcn_readlane(k[i], L);
                const int wh = wk >> 1, wq4 = (wk * wk) >> 2;
                uint32_t tb = 0, tg = 0, tr = 0, tn = 0;
                for (int r = max(y - wh, 0); r <= min(y + wh, rows - 1); r++) {
                    int ca, cb1;
                    disc_span(wq4, r - y, wx, cols, ca, cb1);
                    const uint8_t *row = orig + (size_t)r * op;
                    for (int c = ca + lane; c < cb1; c += 64) { tb += row[3 * (size_t)c]; tg += row[3 * (size_t)c + 1]; tr += row[3 * (size_t)c + 2]; }
                    tn += (uint32_t)(cb1 - ca);
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) { tb += __shfl_xor(tb, m); tg += __shfl_xor(tg, m); tr += __shfl_xor(tr, m); }
                if (lane == L) { sb = tb; sg = tg; sr = tr; sn = tn; }
            }
            if (!local) res = disc_quot(0, sb, sg, sr, sn);
        }
        store_row(art, ap, y, tx0, lane, cols, VEC && tx0 + kDtW <= cols, res);
    }
}

// rtdd_simulate_lens_blur with RTDD_APERTURE_DISC (kernelSize <= 255: effects_api.cpp).  RTDD_OPT_DEFOCUS_PATH as for the box: 0 automatic
// (the tile kernel where its region holds every disc of a depth map), 1 the global table, 2 the tile kernel wherever it fits.
int launch_lens_blur(rtdd_ctx *ctx, const Effect &e) {
    const uint8_t *orig = e.original; const size_t op = e.originalPitch;
    uint8_t *art = e.artistic; const size_t ap = e.artisticPitch;
    const int rows = e.rows, cols = e.cols, kernelSize = e.kernelSize;
    const float *focus_px = pixel_ptr(e.depth, e.depthPitch, e.focusX, e.focusY);      // the pixel form of the focus
    const bool vin = rows_aligned(orig, op), vout = vin && rows_aligned(art, ap);
    if (ctx->opt.defocus_path != 1 && kernelSize / 2 <= kDtHM) {
        const DtGrid t = dt_grid(ctx, rows, cols);
#define RTDD_LT_LAUNCH(V, H) hipLaunchKernelGGL((k_lens_tile<V, H>), t.grid, dim3(256), 0, ctx->stream, orig, op, e.depth, e.depthPitch, art, ap, rows, cols, kernelSize, kernelSize / 2, t.gx, t.ntiles, t.xcd_tiles, e.focusDepth, focus_px)
        if (vout) { if (t.low) RTDD_LT_LAUNCH(true, 16); else RTDD_LT_LAUNCH(true, 24); }
        else { if (t.low) RTDD_LT_LAUNCH(false, 16); else RTDD_LT_LAUNCH(false, 24); }
#undef RTDD_LT_LAUNCH
        RTDD_LAUNCH_CHECK(ctx, "k_lens_tile");
        ctx->defocus_last_path = 2;
        return RTDD_OK;
    }
    // The row prefixes live in the defocus table's buffer.  Their layout is another, and they overwrite what the
    // defocus table keeps zero: its cached geometry is dropped, so the next defocus lays its padding out again.
    const int tpitch = (cols + 1 + 3) / 4 * 4;
    const size_t need = ((size_t)rows * tpitch * sizeof(u64) + 256) / sizeof(uint32_t);
    if (const int st = ensure_sat(ctx, need)) return st;
    ctx->sat_rows = ctx->sat_cols = 0;
    u64 *E = (u64 *)ctx->sat;
    int waves = (tpitch / 4 + 63) / 64; if (waves > 16) waves = 16;
    if (vin) hipLaunchKernelGGL(k_lens_rowprefix<true>, dim3(rows), dim3(64 * waves), 0, ctx->stream, orig, op, E, tpitch, cols);
    else hipLaunchKernelGGL(k_lens_rowprefix<false>, dim3(rows), dim3(64 * waves), 0, ctx->stream, orig, op, E, tpitch, cols);
    RTDD_LAUNCH_CHECK(ctx, "k_lens_rowprefix");
    const LookupGrid t = lookup_grid(ctx, rows, cols, 4, kernelSize / 2, tpitch * sizeof(u64));
    if (vout) hipLaunchKernelGGL(k_lens_gather<true>, t.grid, dim3(256), 0, ctx->stream, orig, op, e.depth, e.depthPitch, E, tpitch, art, ap, rows, cols, kernelSize, t.gx, t.ntiles, t.xcd_tiles, t.strip_w, e.focusDepth, focus_px);
    else hipLaunchKernelGGL(k_lens_gather<false>, t.grid, dim3(256), 0, ctx->stream, orig, op, e.depth, e.depthPitch, E, tpitch, art, ap, rows, cols, kernelSize, t.gx, t.ntiles, t.xcd_tiles, t.strip_w, e.focusDepth, focus_px);
    RTDD_LAUNCH_CHECK(ctx, "k_lens_gather");
    ctx->defocus_last_path = 1;
    ctx->defocus_last_slices = 1;
    return RTDD_OK;
}

}  // namespace rtdd
