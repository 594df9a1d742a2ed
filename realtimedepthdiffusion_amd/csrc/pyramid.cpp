// pyramid.cpp -- the pyramid's images: allocation, lifetime, the setters for image, annotation, guide and regions, what it hands out,
// and the dirty and rebuild flags with the two functions that tell it of reads and writes (pyramid_check_read, pyramid_note_write).
#include <cmath>
#include <new>

#include "pyramid.hpp"

namespace rtdd {

Image image_layout(int rows, int cols, int elem, int images) {
    Image im;
    im.rows = rows; im.cols = cols; im.elem = elem; im.images = images;
    im.pitch = ((size_t)cols * elem + 511) / 512 * 512;       // like cudaMallocPitch: rows padded to 512 B
    im.stride = im.pitch * (size_t)(rows > 0 ? rows : 1);
    return im;
}

int alloc_image(rtdd_ctx *ctx, Image &im, int rows, int cols, int elem, int fill, int images) {
    im = image_layout(rows, cols, elem, images);
    RTDD_HIP(ctx, hipMalloc(&im.ptr, im.bytes()));
    RTDD_HIP(ctx, hipMemsetAsync(im.ptr, fill, im.bytes(), ctx->stream));
    return RTDD_OK;
}

void free_image(Image &im) {
    if (im.ptr) (void)hipFree(im.ptr);
    im = Image();
}

// Every image of `group` (each laid out by image_layout) or none of them; fill >= 0: each filled with that byte on the context's stream
// right behind its allocation.  Out of memory as hipMalloc returns it is RTDD_ERR_NOMEM, any other failure RTDD_ERR_HIP.
static int alloc_group(rtdd_ctx *ctx, const std::vector<Image *> &group, int fill, const char *what) {
    for (Image *im : group) {
        hipError_t e = hipMalloc(&im->ptr, im->bytes());
        int status = e == hipSuccess ? RTDD_OK : e == hipErrorOutOfMemory ? RTDD_ERR_NOMEM : RTDD_ERR_HIP;
        if (e != hipSuccess) im->ptr = nullptr;
        else if (fill >= 0 && (e = hipMemsetAsync(im->ptr, fill, im->bytes(), ctx->stream)) != hipSuccess) status = RTDD_ERR_HIP;
        if (status == RTDD_OK) continue;
        (void)hipGetLastError();                        // (reported here, not again behind the next launch)
        for (Image *q : group) free_image(*q);
        return fail(ctx, status, what, e);
    }
    return RTDD_OK;
}

static bool inside(const Image &im, const void *p) {
    return im.ptr && (const char *)p >= (const char *)im.ptr && (const char *)p < (const char *)im.ptr + im.stride * (size_t)im.images;
}

// Called by the entry points that write an annotation image: is it one of this context's pyramid?  After an uploading live frame the
// pyramid's level-0 scribble / edited images ARE the uploaded staging pair (live.cpp), so a pointer rtdd_pyramid_image handed out
// before that frame names a buffer no estimate reads any more: writing it through the library would lose the strokes silently --
// RTDD_ERR_STATE instead (ask rtdd_pyramid_image again).
static const char *kStaleText = "this level-0 annotation image is no longer the pyramid's: a live frame has uploaded a new pair since "
                                "rtdd_pyramid_image handed the pointer out -- ask rtdd_pyramid_image again";
// (an entry point that only READS annotation images: the same staleness rule)
int pyramid_check_read(rtdd_ctx *ctx, const void *a, const void *b) {
    if (ctx->pyr && (live_stale_pointer(ctx->pyr, a) || live_stale_pointer(ctx->pyr, b))) return fail(ctx, RTDD_ERR_STATE, kStaleText);
    return RTDD_OK;
}
int pyramid_note_write(rtdd_ctx *ctx, const void *scribble, const void *edited, bool erases) {
    Pyramid *p = ctx->pyr;
    if (!p) return RTDD_OK;
    if (live_stale_pointer(p, scribble) || live_stale_pointer(p, edited)) return fail(ctx, RTDD_ERR_STATE, kStaleText);
    // the pyramid's own region pair: a region change -- the code planes are filled again before the next estimate that uses them; the
    // annotation is neither marked as changed nor asked to be rebuilt (an erased region pixel is simply unassigned)
    auto either_in = [&](const Image &s, const Image &e) { return inside(s, scribble) || inside(e, edited) || inside(s, edited) || inside(e, scribble); };
    if (p->has_regions() && either_in(p->region_mask, p->region_edited)) { p->regions_dirty = true; return RTDD_OK; }
    if (erases && p->levels > 0 && (inside(p->scribble[0], scribble) || inside(p->edited[0], edited))) p->annotation_rebuild = true;
    for (int l = 0; l < p->levels; l++)
        if (either_in(p->scribble[l], p->edited[l])) p->annotation_dirty = true;
    // the coarsest depth image carries the injected labels of src/main.cpp:257-259, which an estimate only renews when the annotation
    // changed: whoever overwrites it through the library (rtdd_upload, rtdd_convert_to_float, rtdd_pyrup_depth) makes the next
    // estimate inject again
    if (p->levels > 0 && (inside(p->depth[p->levels - 1], scribble) || inside(p->depth[p->levels - 1], edited))) p->annotation_dirty = true;
    return RTDD_OK;
}

// image b's colour chain: level l from level l - 1, per channel, behind whatever wrote `original` on the context's stream
static int color_chain(rtdd_ctx *ctx, Pyramid *p, int b) {
    for (int l = 1; l < p->levels; l++) {
        const Image &src = l == 1 ? p->original : p->color[l - 1];
        // (level 0 has the image's own size; the levels above it the ceil chain's, as gray[])
        RTDD_TRY(launch_pyrdown_bgr(ctx, (const uint8_t *)src.at(b), src.pitch, l == 1 ? p->rows : src.rows, l == 1 ? p->cols : src.cols,
                                    (uint8_t *)p->color[l].at(b), p->color[l].pitch));
    }
    return RTDD_OK;
}

void pyramid_free(rtdd_ctx *ctx) {
    if (!ctx->pyr) return;
    Pyramid *p = ctx->pyr;
    live_free(p);
    free_image(p->original); free_image(p->depth_u8); free_image(p->artistic); free_image(p->region_edited); free_image(p->region_mask);
    for (auto *v : {&p->gray, &p->scribble, &p->edited, &p->depth, &p->color, &p->region_code})
        for (auto &im : *v) free_image(im);
    delete p;
    ctx->pyr = nullptr;
}

}  // namespace rtdd

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

int rtdd_pyramid_levels(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    const int m = rows < cols ? rows : cols;
    return (int)(log2((double)((m / 45) > 1 ? (m / 45) : 1)) + 1);          // src/main.cpp:95 (integer /45)
}

int rtdd_pyramid_create(rtdd_ctx *ctx, int rows, int cols) { return rtdd_pyramid_create_batch(ctx, rows, cols, 1); }

int rtdd_pyramid_batch(rtdd_ctx *ctx) { return ctx && ctx->pyr ? ctx->pyr->images : 0; }

int rtdd_pyramid_select(rtdd_ctx *ctx, int index) {
    REQUIRE_PYRAMID(ctx);
    REQUIRE(ctx, index >= 0 && index < ctx->pyr->images, "image index outside the batch");
    REQUIRE(ctx, rtdd_live_pending(ctx) == 0, "live frames are in flight");
    ctx->pyr->sel = index;
    return RTDD_OK;
}

int rtdd_pyramid_create_batch(rtdd_ctx *ctx, int rows, int cols, int images) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, rows > 0 && cols > 0, "rows and cols must be positive");
    REQUIRE(ctx, images >= 1 && images <= 4096, "the batch must hold 1..4096 images");
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pyramid_free(ctx);
    Pyramid *p = new (std::nothrow) Pyramid();
    if (!p) return fail(ctx, RTDD_ERR_NOMEM, "pyramid");
    ctx->pyr = p;
    p->rows = rows; p->cols = cols; p->levels = rtdd_pyramid_levels(rows, cols); p->images = images;
    p->level_info.assign(p->levels, rtdd_solve_info{}); p->level_launch_images.assign(p->levels, 0);
    p->gray.resize(p->levels); p->scribble.resize(p->levels); p->edited.resize(p->levels); p->depth.resize(p->levels);
    RTDD_TRY(alloc_image(ctx, p->original, rows, cols, 3, 0, images));
    RTDD_TRY(alloc_image(ctx, p->artistic, rows, cols, 3, 0, images));
    RTDD_TRY(alloc_image(ctx, p->depth_u8, rows, cols, 1, 255, images));
    int gr = rows, gc = cols;
    for (int l = 0; l < p->levels; l++) {
        const int lr = (int)(rows / powf(2, l)), lc = (int)(cols / powf(2, l));   // src/main.cpp:103,129
        RTDD_TRY(alloc_image(ctx, p->gray[l], gr, gc, 1, 0, images));             // ceil chain
        RTDD_TRY(alloc_image(ctx, p->scribble[l], lr, lc, 1, 0, images));         // :132-133
        RTDD_TRY(alloc_image(ctx, p->edited[l], lr, lc, 3, 0, images));           // :130-131
        RTDD_TRY(alloc_image(ctx, p->depth[l], lr, lc, 4, 0, images));
        for (int b = 0; b < images && lr > 0 && lc > 0; b++)                      // :136
            RTDD_TRY(launch_fill_f32(ctx, (float *)p->depth[l].at(b), p->depth[l].pitch, lr, lc, 255.0f));
        gr = (gr + 1) / 2; gc = (gc + 1) / 2;
    }
    ctx->alloc_images = images;
    return rtdd_allocate(ctx, rows, cols, p->levels);                            // :149 (syncs)
}

int rtdd_pyramid_destroy(rtdd_ctx *ctx) {
    if (!ctx) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pyramid_free(ctx);
    return RTDD_OK;
}

int rtdd_pyramid_set_image(rtdd_ctx *ctx, const uint8_t *bgr, size_t pitch) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, bgr && pitch >= (size_t)p->cols * 3, "bad image");
    DeviceGuard g(ctx->device);
    // (a new image resets the warm-start state a logged estimate ran on)
    RTDD_TRY(settle_pending(ctx));
    const int b = p->sel;                          // (a batched pyramid: the selected image)
    for (const Image *dst : {&p->original, &p->edited[0]})                // (the edited image starts as the original: :158)
        RTDD_HIP(ctx, hipMemcpy2DAsync(dst->at(b), dst->pitch, bgr, pitch, (size_t)p->cols * 3, p->rows, hipMemcpyDeviceToDevice, ctx->stream));
    // A new image is a new problem (the reference loads one image per process, src/main.cpp:93): everything an estimate carries
    // over to the next one -- the depth pyramid it warm-starts from (:136) and the coarse annotation levels, which
    // GPUPyrDownAnnotation only ever adds to -- goes back to its initial state.
    p->annotation_dirty = true;
    if (p->has_regions()) {                        // ... and the image's regions: every pixel unassigned again
        for (const Image *im : {&p->region_mask, &p->region_edited}) RTDD_HIP(ctx, hipMemsetAsync(im->at(b), 0, im->stride, ctx->stream));
        p->regions_dirty = true;
    }
    for (int l = 0; l < p->levels; l++) {
        const Image &sc = p->scribble[l], &ed = p->edited[l], &dp = p->depth[l];
        if (sc.ptr) RTDD_HIP(ctx, hipMemsetAsync(sc.at(b), 0, sc.pitch * sc.rows, ctx->stream));
        if (l > 0 && ed.ptr) RTDD_HIP(ctx, hipMemsetAsync(ed.at(b), 0, ed.pitch * ed.rows, ctx->stream));
        if (dp.rows > 0 && dp.cols > 0) RTDD_TRY(launch_fill_f32(ctx, (float *)dp.at(b), dp.pitch, dp.rows, dp.cols, 255.0f));
    }
    p->image_set = true;
    RTDD_TRY(launch_bgr2gray(ctx, (const uint8_t *)p->original.at(b), p->original.pitch, (uint8_t *)p->gray[0].at(b), p->gray[0].pitch, p->rows, p->cols));
    // the gray pyramid depends on the image only: built once here instead of once per estimate (:241-247)
    for (int l = 1; l < p->levels; l++) {
        const Image &src = p->gray[l - 1];
        RTDD_TRY(launch_pyrdown_u8(ctx, (const uint8_t *)src.at(b), src.pitch, src.rows, src.cols, (uint8_t *)p->gray[l].at(b), p->gray[l].pitch));
    }
    return p->guide == RTDD_GUIDE_BGR ? color_chain(ctx, p, b) : RTDD_OK;
}

int rtdd_pyramid_guide(rtdd_ctx *ctx) { return ctx && ctx->pyr ? ctx->pyr->guide : RTDD_GUIDE_GRAY; }

int rtdd_pyramid_set_guide(rtdd_ctx *ctx, int guideKind) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, guideKind == RTDD_GUIDE_GRAY || guideKind == RTDD_GUIDE_BGR, "unknown guide kind");
    if (guideKind == p->guide) return RTDD_OK;
    if (guideKind == RTDD_GUIDE_GRAY) { p->guide = RTDD_GUIDE_GRAY; return RTDD_OK; }      // (the colour levels stay allocated)
    DeviceGuard g(ctx->device);
    if (p->color.empty() && p->levels > 1) {            // the first request: every coarse level, or none (nothing has been launched yet)
        std::vector<Image> lv(p->levels);
        std::vector<Image *> group;
        for (int l = 1; l < p->levels; l++) { lv[l] = image_layout(p->gray[l].rows, p->gray[l].cols, 3, p->images); group.push_back(&lv[l]); }
        RTDD_TRY(alloc_group(ctx, group, /*fill=*/-1, "hipMalloc(colour guide levels)"));
        p->color.swap(lv);
    }
    // the chain of every image of a batch, from the images as they are now (set_image keeps it up to date only while the guide is BGR)
    if (p->image_set) for (int b = 0; b < p->images; b++) RTDD_TRY(color_chain(ctx, p, b));
    p->guide = RTDD_GUIDE_BGR;
    return RTDD_OK;
}

int rtdd_pyramid_regions(rtdd_ctx *ctx) { return ctx && ctx->pyr ? ctx->pyr->region_flags : 0; }

int rtdd_pyramid_set_regions(rtdd_ctx *ctx, int flags) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, (flags & ~(RTDD_REGION_CUT | RTDD_REGION_SMOOTH)) == 0, "unknown region flag");
    if (flags == 0 || p->has_regions()) { p->region_flags = flags; return RTDD_OK; }       // (0 keeps the images: a host toggles)
    DeviceGuard g(ctx->device);
    // the first request: the level-0 pair and every level's codes, zeroed, per image of a batch -- or none of them
    Image ed = image_layout(p->rows, p->cols, 3, p->images), mk = image_layout(p->rows, p->cols, 1, p->images);
    std::vector<Image> code(p->levels);
    std::vector<Image *> group{&ed, &mk};
    for (int l = 0; l < p->levels; l++) { code[l] = image_layout(p->scribble[l].rows, p->scribble[l].cols, 1, p->images); group.push_back(&code[l]); }
    RTDD_TRY(alloc_group(ctx, group, /*fill=*/0, "hipMalloc(region images)"));
    p->region_edited = ed; p->region_mask = mk; p->region_code.swap(code);
    p->regions_dirty = false;                       // (all zero: the codes of an all-unassigned pair)
    p->region_flags = flags;
    return RTDD_OK;
}

int rtdd_pyramid_regions_changed(rtdd_ctx *ctx) {
    REQUIRE_PYRAMID(ctx);
    if (!ctx->pyr->has_regions()) return fail(ctx, RTDD_ERR_STATE, "the pyramid has no regions: rtdd_pyramid_set_regions first");
    ctx->pyr->regions_dirty = true;
    return RTDD_OK;
}

int rtdd_pyramid_set_annotation(rtdd_ctx *ctx, const uint8_t *annotation, size_t pitch) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, annotation && pitch >= (size_t)p->cols, "bad annotation");
    DeviceGuard g(ctx->device);
    p->annotation_dirty = true;
    return launch_decode_annotation(ctx, (const uint8_t *)p->original.at(p->sel), p->original.pitch, annotation, pitch, (uint8_t *)p->edited[0].at(p->sel),
                                    p->edited[0].pitch, (uint8_t *)p->scribble[0].at(p->sel), p->scribble[0].pitch, p->rows, p->cols);
}

int rtdd_pyramid_image(rtdd_ctx *ctx, int kind, int level, void **ptr, size_t *pitch, int *rows, int *cols) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    const Image *im = nullptr;
    REQUIRE(ctx, level >= 0 && level < p->levels, "level out of range");
    switch (kind) {
        case RTDD_IMG_ORIGINAL: im = level == 0 ? &p->original : nullptr; break;
        case RTDD_IMG_DEPTH_U8: im = level == 0 ? &p->depth_u8 : nullptr; break;
        case RTDD_IMG_ARTISTIC: im = level == 0 ? &p->artistic : nullptr; break;
        case RTDD_IMG_GRAY: im = &p->gray[level]; break;
        case RTDD_IMG_SCRIBBLE: im = &p->scribble[level]; break;
        case RTDD_IMG_EDITED: im = &p->edited[level]; break;
        case RTDD_IMG_DEPTH: im = &p->depth[level]; break;
        case RTDD_IMG_GUIDE_BGR:
            if (level > 0 && p->color.empty()) return fail(ctx, RTDD_ERR_STATE, "the colour guide's coarse levels do not exist: rtdd_pyramid_set_guide(RTDD_GUIDE_BGR) first");
            im = level == 0 ? &p->original : &p->color[level];
            break;
        case RTDD_IMG_REGION_EDITED: case RTDD_IMG_REGION_MASK: case RTDD_IMG_REGION_CODE:
            if (!p->has_regions()) return fail(ctx, RTDD_ERR_STATE, "the pyramid has no regions: rtdd_pyramid_set_regions first");
            im = kind == RTDD_IMG_REGION_CODE ? &p->region_code[level] : level != 0 ? nullptr : kind == RTDD_IMG_REGION_EDITED ? &p->region_edited : &p->region_mask;
            break;
        default: break;
    }
    REQUIRE(ctx, im != nullptr, "no such pyramid image");
    if (ptr) *ptr = im->at(p->sel);
    if (pitch) *pitch = im->pitch;
    if (rows) *rows = im->rows;
    if (cols) *cols = im->cols;
    return RTDD_OK;
}

int rtdd_pyramid_level_info(rtdd_ctx *ctx, int level, rtdd_solve_info *info, int *imagesPerLaunch) {
    if (!info) return RTDD_ERR_INVALID;
    REQUIRE_PYRAMID(ctx);
    REQUIRE(ctx, level >= 0 && level < ctx->pyr->levels, "level out of range");
    *info = ctx->pyr->level_info[level];
    if (imagesPerLaunch) *imagesPerLaunch = ctx->pyr->level_launch_images[level];
    return RTDD_OK;
}

int rtdd_pyramid_annotation_rebuild(rtdd_ctx *ctx) {
    REQUIRE_PYRAMID(ctx);
    ctx->pyr->annotation_dirty = true; ctx->pyr->annotation_rebuild = true;
    return RTDD_OK;
}

int rtdd_pyramid_annotation_changed(rtdd_ctx *ctx) {
    REQUIRE_PYRAMID(ctx);
    ctx->pyr->annotation_dirty = true;
    return RTDD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
