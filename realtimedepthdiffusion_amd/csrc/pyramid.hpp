// pyramid.hpp -- the state of the whole-estimate driver (include/rtdd.h; /root/reference/src/main.cpp:92-155 setup, :232-295 estimate)
// and what its three units -- pyramid.cpp, estimate.cpp, live.cpp -- call in each other.  Host only: no .hip file includes it.
#pragma once

#include "rtdd_internal.hpp"

namespace rtdd {

struct Image {
    void *ptr = nullptr;
    size_t pitch = 0;
    int rows = 0, cols = 0, elem = 1;
    // a batched pyramid (rtdd_pyramid_create_batch) holds every image `images` times, copy b `stride` bytes behind copy b - 1
    size_t stride = 0;
    int images = 1;
    void *at(int b) const { return ptr ? (char *)ptr + (size_t)b * stride : nullptr; }
    size_t bytes() const { return stride * (size_t)images; }
};

struct Pyramid {
    int levels = 0, rows = 0, cols = 0;
    Image original, depth_u8, artistic;
    std::vector<Image> gray, scribble, edited, depth;
    // The colour guide (rtdd_pyramid_set_guide): while `guide` is RTDD_GUIDE_BGR the per-level solves read level l's colour image instead
    // of gray[l].  color[l], l >= 1: cv::pyrDown per channel of level l - 1, the ceil-sized chain of gray[]; level 0 is `original` itself
    // (color[0] stays empty).  Allocated by the first request for BGR, kept from then on; a pyramid that never asks has none.
    int guide = RTDD_GUIDE_GRAY;
    std::vector<Image> color;
    bool image_set = false;               // rtdd_pyramid_set_image has been called: there is something to build the chain from
    // Depth regions (rtdd_pyramid_set_regions): a second level-0 pair the paint calls write like the annotation's -- the label is the
    // region id -- and one u8 code plane per level (the floor chain, like scribble[]) which k_region_codes fills from it, all levels in
    // one launch, before the first estimate after the pair changed.  While region_flags != 0 the per-level solves apply the flags with
    // level l's codes.  Allocated zeroed by the first non-zero request, kept from then on; a pyramid that never asks has none.
    int region_flags = 0;
    Image region_edited, region_mask;
    std::vector<Image> region_code;
    bool regions_dirty = false;           // (of ANY image of a batch: the launch covers them all)
    bool has_regions() const { return region_mask.ptr != nullptr; }
    const Image &guide_image(int kind, int l) const { return kind != RTDD_GUIDE_BGR ? gray[l] : l == 0 ? original : color[l]; }
    // The coarse annotation levels and the coarsest level's injection depend on the annotation only (src/main.cpp:249-259;
    // GPUPyrDownAnnotation only ever adds, SURVEY A.8, and the solver never moves a Dirichlet pixel): they are brought up to date
    // by the first estimate after the annotation changed, not by every estimate.
    bool annotation_dirty = true;         // (of ANY image of a batch: bringing an up-to-date image up to date again changes nothing)
    // rtdd_pyramid_annotation_rebuild / an erasing rtdd_paint_strokes: labels were removed, so the next estimate builds the coarse levels
    // as if they had been all zero instead of adding to them (every image of a batch: a rebuilt image that lost nothing is what it was)
    bool annotation_rebuild = false;
    int images = 1, sel = 0;              // batch size; the image the single-image entry points address (rtdd_pyramid_select)
    std::vector<rtdd_solve_info> level_info;      // what the most recent estimate ran per level (rtdd_pyramid_level_info)
    std::vector<int> level_launch_images;
    struct Live *live = nullptr;          // rtdd_live_submit's second stream, staging images and events (created on first use; live.cpp)
};

// ---- pyramid.cpp ----
// where rows x cols elements of `elem` bytes go, `images` times over: like cudaMallocPitch, rows padded to 512 B (ptr stays null)
Image image_layout(int rows, int cols, int elem, int images = 1);
// ... allocated, and filled with the byte `fill` on the context's stream
int alloc_image(rtdd_ctx *ctx, Image &im, int rows, int cols, int elem, int fill, int images = 1);
void free_image(Image &im);

// ---- estimate.cpp ----
// whole_batch: every image of the context's (batched) pyramid in the same launches; else the selected one.
// live: a live frame's own images (its annotation pair, the second target of its u8 map, its depth effect); default: not a live frame.
int estimate_submit(rtdd_ctx *ctx, int maxIterations, unsigned long long *op_id, bool whole_batch, const LiveTargets &live);

// ---- live.cpp ----
void live_free(Pyramid *p);               // (puts the pyramid's own level-0 annotation pair and artistic image back)
// q lies in a level-0 annotation image that a live frame has since replaced (pyramid_note_write, pyramid_check_read)
bool live_stale_pointer(const Pyramid *p, const void *q);

}  // namespace rtdd
