// image_api.cpp -- the entry points that work on images they are handed and keep no pyramid state: the spelt-out cascade's image steps,
// the paint and fill calls, host <-> device copies (with the bounce copies for an unaligned host pitch), page-locked host memory.
#include <cmath>

#include "rtdd_internal.hpp"

namespace rtdd {

static int bounce_reserve(rtdd_ctx *ctx, Bounce &b, size_t bytes, hipStream_t stream) {
    if (b.bytes >= bytes) return RTDD_OK;
    if (b.ptr) { RTDD_HIP(ctx, hipStreamSynchronize(stream)); RTDD_HIP(ctx, hipFree(b.ptr)); b.ptr = nullptr; b.bytes = 0; }
    RTDD_HIP(ctx, hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    return RTDD_OK;
}
int copy_h2d_linear(rtdd_ctx *ctx, Bounce &b, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows,
    hipStream_t copyStream, hipStream_t kernelStream) {
    if (wants_bounce(hostPitch, widthBytes, rows)) {
        RTDD_TRY(bounce_reserve(ctx, b, widthBytes * (size_t)rows, kernelStream));
        RTDD_HIP(ctx, hipMemcpyAsync(b.ptr, host, widthBytes * (size_t)rows, hipMemcpyHostToDevice, copyStream));
    } else RTDD_HIP(ctx, hipMemcpy2DAsync(dev, devPitch, host, hostPitch, widthBytes, rows, hipMemcpyHostToDevice, copyStream));
    return RTDD_OK;
}
int copy_h2d_repitch(rtdd_ctx *ctx, const Bounce &b, void *dev, size_t devPitch, size_t hostPitch, size_t widthBytes, int rows, hipStream_t kernelStream) {
    if (!wants_bounce(hostPitch, widthBytes, rows)) return RTDD_OK;
    return launch_repitch(ctx, kernelStream, b.ptr, widthBytes, dev, devPitch, widthBytes, rows);
}
int copy_h2d(rtdd_ctx *ctx, Bounce &b, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows, hipStream_t stream) {
    RTDD_TRY(copy_h2d_linear(ctx, b, dev, devPitch, host, hostPitch, widthBytes, rows, stream, stream));
    return copy_h2d_repitch(ctx, b, dev, devPitch, hostPitch, widthBytes, rows, stream);
}
int copy_d2h(rtdd_ctx *ctx, Bounce &b, void *host, size_t hostPitch, const void *dev, size_t devPitch, size_t widthBytes, int rows, hipStream_t stream) {
    if (wants_bounce(hostPitch, widthBytes, rows)) {
        RTDD_TRY(bounce_reserve(ctx, b, widthBytes * (size_t)rows, stream));
        RTDD_TRY(launch_repitch(ctx, stream, dev, devPitch, b.ptr, widthBytes, widthBytes, rows));
        RTDD_HIP(ctx, hipMemcpyAsync(host, b.ptr, widthBytes * (size_t)rows, hipMemcpyDeviceToHost, stream));
    } else RTDD_HIP(ctx, hipMemcpy2DAsync(host, hostPitch, dev, devPitch, widthBytes, rows, hipMemcpyDeviceToHost, stream));
    return RTDD_OK;
}

}  // namespace rtdd

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

int rtdd_convert_to_float(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, float *dst, size_t dstPitch,
                          const uint8_t *mask, size_t maskPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, src && dst && mask, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    REQUIRE(ctx, f32_image_aligned(dst, dstPitch), kF32AlignText);
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, srcPitch >= (size_t)cols * 3 && dstPitch >= (size_t)cols * 4 && maskPitch >= (size_t)cols, "pitch smaller than a row");
    DeviceGuard g(ctx->device);
    // (the coarsest depth image of the context's pyramid? then the next estimate injects again; stale annotation pointers: RTDD_ERR_STATE)
    RTDD_TRY(pyramid_check_read(ctx, src, mask));
    RTDD_TRY(pyramid_note_write(ctx, dst, dst));
    return launch_convert(ctx, src, srcPitch, dst, dstPitch, mask, maskPitch, rows, cols);
}

int rtdd_pyrdown_annotation(rtdd_ctx *ctx, const uint8_t *prevScribble, size_t prevScribblePitch, const uint8_t *prevEdited,
                            size_t prevEditedPitch, int previousRows, int previousCols, uint8_t *currScribble,
                            size_t currScribblePitch, uint8_t *currEdited, size_t currEditedPitch, int currentRows, int currentCols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, prevScribble && prevEdited && currScribble && currEdited, "null image pointer");
    REQUIRE(ctx, previousRows >= 0 && previousCols >= 0 && currentRows >= 0 && currentCols >= 0, "negative size");
    if (currentRows == 0 || currentCols == 0) return RTDD_OK;
    REQUIRE(ctx, prevScribblePitch >= (size_t)previousCols && prevEditedPitch >= (size_t)previousCols * 3 &&
                 currScribblePitch >= (size_t)currentCols && currEditedPitch >= (size_t)currentCols * 3, "pitch smaller than a row");
    DeviceGuard g(ctx->device);
    RTDD_TRY(pyramid_check_read(ctx, prevScribble, prevEdited));
    RTDD_TRY(pyramid_note_write(ctx, currScribble, currEdited));
    return launch_pyrdown_annotation(ctx, prevScribble, prevScribblePitch, prevEdited, prevEditedPitch, previousRows, previousCols,
                                     currScribble, currScribblePitch, currEdited, currEditedPitch, currentRows, currentCols);
}

int rtdd_paint_image(rtdd_ctx *ctx, int x, int y, int scribbleColor, int scribbleRadius, uint8_t *edited, size_t editedPitch,
                     uint8_t *scribble, size_t scribblePitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, edited && scribble, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, editedPitch >= (size_t)cols * 3 && scribblePitch >= (size_t)cols, "pitch smaller than a row");
    DeviceGuard g(ctx->device);
    RTDD_TRY(pyramid_note_write(ctx, scribble, edited));
    return launch_paint(ctx, x, y, scribbleColor, scribbleRadius, PaintTarget{edited, editedPitch, scribble, scribblePitch, nullptr, 0, rows, cols});
}

// ---- rtdd_paint_strokes, rtdd_paint_ramp_strokes, rtdd_fill_polygon, rtdd_fill_similar: what they share ----
// A call checks its own records first (they say whether it erases), then its target; an empty image or no record is RTDD_OK before any
// pitch is looked at; then, with the device set, begin_paint.
static int check_paint_target(rtdd_ctx *ctx, const PaintTarget &t, bool erases) {
    REQUIRE(ctx, t.edited && t.scribble, "null image pointer");
    REQUIRE(ctx, t.rows >= 0 && t.cols >= 0, "negative size");
    REQUIRE(ctx, t.rows <= 32768 && t.cols <= 32768, "image larger than 32768 pixels in a direction");
    REQUIRE(ctx, !erases || t.original, "an erasing stroke or fill needs the original image");
    return RTDD_OK;
}

// The pitches, and the pyramid hears of the write: an eraser on its own level-0 pair makes the next estimate build the coarse levels,
// which otherwise only accumulate, afresh.  Nothing goes into the pending-call log -- a paint call cannot time out, and an estimate that
// is run again reads the images as the paint calls in front of it left them.
static int begin_paint(rtdd_ctx *ctx, const PaintTarget &t, bool erases) {
    REQUIRE(ctx, t.editedPitch >= (size_t)t.cols * 3 && t.scribblePitch >= (size_t)t.cols && (!erases || t.originalPitch >= (size_t)t.cols * 3),
        "pitch smaller than a row");
    return pyramid_note_write(ctx, t.scribble, t.edited, erases);
}

// what the stroke calls and rtdd_ramp_polyline refuse in a record's geometry
static bool stroke_geometry_ok(int x0, int y0, int x1, int y1, int radius, int brush, const char **why) {
    for (int v : {x0, y0, x1, y1})
        if (v < -32768 || v > 32767) { *why = "stroke endpoint outside [-32768, 32767]"; return false; }
    if (radius < 0 || radius > 1024) { *why = "stroke radius outside [0, 1024]"; return false; }
    if (brush != RTDD_BRUSH_SQUARE && brush != RTDD_BRUSH_ROUND) { *why = "unknown brush"; return false; }
    return true;
}

// ... and in the two labels of a ramp stroke or a fill
static bool label_pair_ok(int label0, int label1, const char **why) {
    if (label0 < RTDD_STROKE_ERASE || label0 > 255 || label1 < RTDD_STROKE_ERASE || label1 > 255) { *why = "label outside [-1, 255]"; return false; }
    if ((label0 == RTDD_STROKE_ERASE) != (label1 == RTDD_STROKE_ERASE)) { *why = "one label of a ramp or a fill erases and the other paints"; return false; }
    return true;
}

int rtdd_paint_strokes(rtdd_ctx *ctx, const rtdd_stroke *strokes, int count, uint8_t *edited, size_t editedPitch, uint8_t *scribble,
                       size_t scribblePitch, const uint8_t *original, size_t originalPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, original, originalPitch, rows, cols};
    REQUIRE(ctx, count >= 0 && count <= 4096, "count outside [0, 4096]");
    REQUIRE(ctx, strokes || count == 0, "null stroke array");
    bool erases = false;
    const char *why = nullptr;
    for (int i = 0; i < count; i++) {
        const rtdd_stroke &q = strokes[i];
        REQUIRE(ctx, stroke_geometry_ok(q.x0, q.y0, q.x1, q.y1, q.radius, q.brush, &why), why);
        REQUIRE(ctx, q.label >= RTDD_STROKE_ERASE && q.label <= 255, "stroke label outside [-1, 255]");
        erases = erases || q.label == RTDD_STROKE_ERASE;
    }
    RTDD_TRY(check_paint_target(ctx, t, erases));
    if (rows == 0 || cols == 0 || count == 0) return RTDD_OK;
    DeviceGuard g(ctx->device);
    RTDD_TRY(begin_paint(ctx, t, erases));
    return launch_paint_strokes(ctx, strokes, count, t);
}

int rtdd_paint_ramp_strokes(rtdd_ctx *ctx, const rtdd_ramp_stroke *strokes, int count, uint8_t *edited, size_t editedPitch, uint8_t *scribble,
                            size_t scribblePitch, const uint8_t *original, size_t originalPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, original, originalPitch, rows, cols};
    REQUIRE(ctx, count >= 0 && count <= 4096, "count outside [0, 4096]");
    REQUIRE(ctx, strokes || count == 0, "null stroke array");
    bool erases = false;
    const char *why = nullptr;
    for (int i = 0; i < count; i++) {
        const rtdd_ramp_stroke &q = strokes[i];
        REQUIRE(ctx, stroke_geometry_ok(q.x0, q.y0, q.x1, q.y1, q.radius, q.brush, &why), why);
        REQUIRE(ctx, label_pair_ok(q.label0, q.label1, &why), why);
        erases = erases || q.label0 == RTDD_STROKE_ERASE;
    }
    RTDD_TRY(check_paint_target(ctx, t, erases));
    if (rows == 0 || cols == 0 || count == 0) return RTDD_OK;
    DeviceGuard g(ctx->device);
    RTDD_TRY(begin_paint(ctx, t, erases));
    return launch_paint_strokes(ctx, strokes, count, t);
}

int rtdd_fill_polygon(rtdd_ctx *ctx, const int *xy, int n, const rtdd_fill *fill, uint8_t *edited, size_t editedPitch, uint8_t *scribble,
                      size_t scribblePitch, const uint8_t *original, size_t originalPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, original, originalPitch, rows, cols};
    REQUIRE(ctx, fill, "null fill");
    REQUIRE(ctx, n >= 0 && n <= 768, "n outside [0, 768]");
    REQUIRE(ctx, xy || n == 0, "null vertex array");
    REQUIRE(ctx, fill->rule == RTDD_FILL_NONZERO || fill->rule == RTDD_FILL_EVEN_ODD, "unknown fill rule");
    for (int i = 0; i < 2 * n; i++) REQUIRE(ctx, xy[i] >= -32768 && xy[i] <= 32767, "vertex coordinate outside [-32768, 32767]");
    for (int v : {fill->ax0, fill->ay0, fill->ax1, fill->ay1}) REQUIRE(ctx, v >= -32768 && v <= 32767, "axis coordinate outside [-32768, 32767]");
    const char *why = nullptr;
    REQUIRE(ctx, label_pair_ok(fill->label0, fill->label1, &why), why);
    const bool erases = fill->label0 == RTDD_STROKE_ERASE;
    RTDD_TRY(check_paint_target(ctx, t, erases));
    if (rows == 0 || cols == 0 || n == 0) return RTDD_OK;
    DeviceGuard g(ctx->device);
    RTDD_TRY(begin_paint(ctx, t, erases));
    return launch_fill_polygon(ctx, xy, n, *fill, t);
}

// The one paint call that synchronises (the number of grow passes depends on the data) and the one that always reads the original.
int rtdd_fill_similar(rtdd_ctx *ctx, const rtdd_wand *wand, uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *original, size_t originalPitch, int rows, int cols, rtdd_wand_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, original, originalPitch, rows, cols};
    REQUIRE(ctx, wand, "null wand");
    REQUIRE(ctx, wand->tolerance >= 0 && wand->tolerance <= 255, "tolerance outside [0, 255]");
    REQUIRE(ctx, (wand->flags & ~(RTDD_WAND_CONNECT_8 | RTDD_WAND_GLOBAL)) == 0, "unknown wand flag");
    for (int v : {wand->ax0, wand->ay0, wand->ax1, wand->ay1}) REQUIRE(ctx, v >= -32768 && v <= 32767, "axis coordinate outside [-32768, 32767]");
    const char *why = nullptr;
    REQUIRE(ctx, label_pair_ok(wand->label0, wand->label1, &why), why);
    REQUIRE(ctx, original, "null original image: it is what \"similar\" reads");
    RTDD_TRY(check_paint_target(ctx, t, false));
    REQUIRE(ctx, wand->x >= 0 && wand->x < cols && wand->y >= 0 && wand->y < rows, "the seed lies outside the image (an empty image has no seed)");
    REQUIRE(ctx, editedPitch >= (size_t)cols * 3 && scribblePitch >= (size_t)cols && originalPitch >= (size_t)cols * 3, "pitch smaller than a row");
    const bool erases = wand->label0 == RTDD_STROKE_ERASE;
    DeviceGuard g(ctx->device);
    // the call synchronises the stream: confirm (or heal) the logged solves and estimates through their own path first, while the state
    // they ran on still exists -- and before the pyramid hears of this write, which a replayed estimate would otherwise take for its own;
    // the synchronisations behind that are plain.  Not logged itself, like every paint call.
    RTDD_TRY(settle_pending(ctx));
    RTDD_TRY(begin_paint(ctx, t, erases));
    return launch_fill_similar(ctx, *wand, t, info);
}

// rtdd_fill_similar's sibling on the depth map: synchronises for the same reason, and reads `original` only when it erases.
int rtdd_fill_surface(rtdd_ctx *ctx, const rtdd_surface_wand *wand, uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch, int rows, int cols,
                      rtdd_wand_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, original, originalPitch, rows, cols};
    REQUIRE(ctx, wand, "null wand");
    for (float v : {wand->step, wand->below, wand->above})
        REQUIRE(ctx, std::isfinite(v) && v >= 0.0f && v <= 255.0f, "step, below or above not a finite value in [0, 255]");
    REQUIRE(ctx, (wand->flags & ~RTDD_SURFACE_GLOBAL) == 0, "unknown surface wand flag");
    for (int v : {wand->ax0, wand->ay0, wand->ax1, wand->ay1}) REQUIRE(ctx, v >= -32768 && v <= 32767, "axis coordinate outside [-32768, 32767]");
    const char *why = nullptr;
    REQUIRE(ctx, label_pair_ok(wand->label0, wand->label1, &why), why);
    const bool erases = wand->label0 == RTDD_STROKE_ERASE;
    REQUIRE(ctx, depth, "null depth map: it is what the surface wand reads");
    RTDD_TRY(check_paint_target(ctx, t, erases));
    REQUIRE(ctx, wand->x >= 0 && wand->x < cols && wand->y >= 0 && wand->y < rows, "the seed lies outside the image (an empty image has no seed)");
    REQUIRE(ctx, depthPitch >= (size_t)cols * 4, "pitch smaller than a row");
    REQUIRE(ctx, f32_image_aligned(depth, depthPitch), kF32AlignText);
    REQUIRE(ctx, editedPitch >= (size_t)cols * 3 && scribblePitch >= (size_t)cols && (!erases || originalPitch >= (size_t)cols * 3), "pitch smaller than a row");
    DeviceGuard g(ctx->device);
    // (as rtdd_fill_similar; here it is also what makes the depth map final: it is usually the output of an estimate still in the log)
    RTDD_TRY(settle_pending(ctx));
    RTDD_TRY(begin_paint(ctx, t, erases));
    return launch_fill_surface(ctx, *wand, t, depth, depthPitch, info);
}

// Every component of rtdd_fill_surface's link graph in one call: synchronises for the counts and records, settles first for
// rtdd_fill_surface's reason.  Everything is checked before the device is touched.
int rtdd_segment_surfaces(rtdd_ctx *ctx, const rtdd_segmentation *seg, uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                          const float *depth, size_t depthPitch, int32_t *labels, size_t labelsPitch, int rows, int cols, rtdd_segment *segments,
                          rtdd_segment_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    const PaintTarget t{edited, editedPitch, scribble, scribblePitch, nullptr, 0, rows, cols};
    REQUIRE(ctx, seg, "null segmentation");
    for (float v : {seg->step, seg->lo, seg->hi}) REQUIRE(ctx, std::isfinite(v) && v >= 0.0f && v <= 255.0f, "step, lo or hi not a finite value in [0, 255]");
    REQUIRE(ctx, seg->lo <= seg->hi, "lo above hi");
    REQUIRE(ctx, seg->minPixels >= 1, "minPixels below 1");
    REQUIRE(ctx, seg->maxRegions >= 1 && seg->maxRegions <= 255, "maxRegions outside [1, 255]");
    REQUIRE(ctx, seg->firstCode >= 1 && seg->firstCode <= 255 && seg->firstCode + seg->maxRegions - 1 <= 255, "the codes firstCode .. firstCode + maxRegions - 1 leave [1, 255]");
    REQUIRE(ctx, seg->flags == 0, "unknown segmentation flag");
    REQUIRE(ctx, depth, "null depth map: it is what the segmentation reads");
    REQUIRE(ctx, (edited != nullptr) == (scribble != nullptr), "one image of the pair given without the other");
    REQUIRE(ctx, rows >= 1 && cols >= 1, "an empty image, or a negative size");
    REQUIRE(ctx, rows <= 32768 && cols <= 32768, "image larger than 32768 pixels in a direction");
    REQUIRE(ctx, depthPitch >= (size_t)cols * 4, "pitch smaller than a row");
    REQUIRE(ctx, f32_image_aligned(depth, depthPitch), kF32AlignText);
    REQUIRE(ctx, !edited || (editedPitch >= (size_t)cols * 3 && scribblePitch >= (size_t)cols), "pitch smaller than a row");
    REQUIRE(ctx, !labels || (labelsPitch >= (size_t)cols * 4 && (uintptr_t)labels % 4 == 0 && labelsPitch % 4 == 0),
            "the label map needs a pitch of at least 4 * cols and a pointer and a pitch that are multiples of 4");
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));                                   // (as rtdd_fill_surface)
    if (edited) RTDD_TRY(begin_paint(ctx, t, false));
    return launch_segment_surfaces(ctx, *seg, t, depth, depthPitch, labels, labelsPitch, segments, info);
}

// host arithmetic only (include/rtdd.h has the rule): doubles, every operation rounded on its own
int rtdd_ramp_polyline(const int *xy, int n, int radius, int brush, int label0, int label1, rtdd_ramp_stroke *out) {
#pragma clang fp contract(off)
    if (!xy || !out || n < 1 || n > 4097) return RTDD_ERR_INVALID;
    if (label0 < 0 || label0 > 255 || label1 < 0 || label1 > 255) return RTDD_ERR_INVALID;
    const char *why = nullptr;
    for (int i = 0; i < n; i++)
        if (!stroke_geometry_ok(xy[2 * i], xy[2 * i + 1], xy[2 * i], xy[2 * i + 1], radius, brush, &why)) return RTDD_ERR_INVALID;
    if (n == 1) { out[0] = rtdd_ramp_stroke{xy[0], xy[1], xy[0], xy[1], radius, brush, label0, label0}; return RTDD_OK; }
    std::vector<double> s((size_t)n);
    s[0] = 0.0;
    for (int i = 1; i < n; i++) {
        const long long dx = (long long)xy[2 * i] - xy[2 * i - 2], dy = (long long)xy[2 * i + 1] - xy[2 * i - 1];
        s[i] = s[i - 1] + std::sqrt((double)(dx * dx + dy * dy));
    }
    const double S = s[n - 1];
    auto label = [&](int i) {
        if (!(S > 0.0)) return label0;
        const double share = s[i] / S, rise = (double)(label1 - label0) * share, at = (double)label0 + rise;
        return (int)std::floor(at + 0.5);
    };
    int prev = label(0);
    for (int i = 0; i + 1 < n; i++) {
        const int next = label(i + 1);
        out[i] = rtdd_ramp_stroke{xy[2 * i], xy[2 * i + 1], xy[2 * i + 2], xy[2 * i + 3], radius, brush, prev, next};
        prev = next;
    }
    return RTDD_OK;
}

int rtdd_bgr2gray(rtdd_ctx *ctx, const uint8_t *bgr, size_t bgrPitch, uint8_t *gray, size_t grayPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, bgr && gray && rows > 0 && cols > 0 && bgrPitch >= (size_t)cols * 3 && grayPitch >= (size_t)cols, "bad argument");
    DeviceGuard g(ctx->device);
    return launch_bgr2gray(ctx, bgr, bgrPitch, gray, grayPitch, rows, cols);
}

int rtdd_pyrdown_gray(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, int rows, int cols, uint8_t *dst, size_t dstPitch) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, src && dst && rows > 0 && cols > 0 && srcPitch >= (size_t)cols && dstPitch >= (size_t)((cols + 1) / 2), "bad argument");
    DeviceGuard g(ctx->device);
    return launch_pyrdown_u8(ctx, src, srcPitch, rows, cols, dst, dstPitch);
}

int rtdd_pyrdown_bgr(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, int rows, int cols, uint8_t *dst, size_t dstPitch) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, src && dst && rows > 0 && cols > 0 && srcPitch >= (size_t)cols * 3 && dstPitch >= (size_t)((cols + 1) / 2) * 3, "bad argument");
    DeviceGuard g(ctx->device);
    return launch_pyrdown_bgr(ctx, src, srcPitch, rows, cols, dst, dstPitch);
}

int rtdd_pyrup_depth(rtdd_ctx *ctx, const float *src, size_t srcPitch, int rows, int cols, float *dst, size_t dstPitch, int dstRows, int dstCols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, src && dst && rows > 0 && cols > 0 && dstRows > 0 && dstCols > 0 && srcPitch >= (size_t)cols * 4 && dstPitch >= (size_t)dstCols * 4, "bad argument");
    REQUIRE(ctx, f32_image_aligned(src, srcPitch) && f32_image_aligned(dst, dstPitch), kF32AlignText);
    DeviceGuard g(ctx->device);
    // (as rtdd_index_to_weight: `src` may be the output of a logged solve whose persistent launch gave up -- the spelt-out cascade,
    // solve -> pyrUp -> inject -> solve, queued asynchronously)
    RTDD_TRY(settle_pending(ctx));
    RTDD_TRY(pyramid_note_write(ctx, dst, dst));
    return launch_pyrup_inject(ctx, src, srcPitch, rows, cols, dst, dstPitch, dstRows, dstCols, nullptr, 0, nullptr, 0);
}

int rtdd_depth_to_u8(rtdd_ctx *ctx, const float *src, size_t srcPitch, uint8_t *dst, size_t dstPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, src && dst && rows > 0 && cols > 0 && srcPitch >= (size_t)cols * 4 && dstPitch >= (size_t)cols, "bad argument");
    REQUIRE(ctx, f32_image_aligned(src, srcPitch), kF32AlignText);
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));     // (as rtdd_pyrup_depth)
    return launch_depth_to_u8(ctx, src, srcPitch, dst, dstPitch, rows, cols);
}

int rtdd_upload(rtdd_ctx *ctx, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, dev && host && rows >= 0 && devPitch >= widthBytes && hostPitch >= widthBytes, "bad argument");
    DeviceGuard g(ctx->device);
    // the destination may be an input of a logged call that still has to be run again: settle first (this call synchronises anyway)
    RTDD_TRY(settle_pending(ctx));
    RTDD_TRY(pyramid_note_write(ctx, dev, dev));
    RTDD_TRY(copy_h2d(ctx, ctx->bounce, dev, devPitch, host, hostPitch, widthBytes, rows, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTDD_OK;
}

int rtdd_download(rtdd_ctx *ctx, void *host, size_t hostPitch, const void *dev, size_t devPitch, size_t widthBytes, int rows) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, dev && host && rows >= 0 && devPitch >= widthBytes && hostPitch >= widthBytes, "bad argument");
    DeviceGuard g(ctx->device);
    RTDD_TRY(copy_d2h(ctx, ctx->bounce, host, hostPitch, dev, devPitch, widthBytes, rows, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int heals = ctx->heals;
    const int rc = check_persistent_status(ctx);  // what was just downloaded may come from a persistent launch that gave up ...
    if (rc != RTDD_OK || ctx->heals == heals) return rc;
    // ... and has been run again since
    RTDD_TRY(copy_d2h(ctx, ctx->bounce, host, hostPitch, dev, devPitch, widthBytes, rows, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTDD_OK;
}

int rtdd_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return RTDD_ERR_INVALID;
    *ptr = nullptr;
    return hipHostMalloc(ptr, bytes > 0 ? bytes : 1, hipHostMallocDefault) == hipSuccess ? RTDD_OK : RTDD_ERR_NOMEM;
}

int rtdd_host_free(void *ptr) { return !ptr || hipHostFree(ptr) == hipSuccess ? RTDD_OK : RTDD_ERR_HIP; }

}  // extern "C"
#pragma GCC visibility pop
