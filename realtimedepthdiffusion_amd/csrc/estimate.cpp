// estimate.cpp -- the whole estimate on the context's pyramid (src/main.cpp:239-291): the annotation pyramid and the region codes, the
// per-level solves with the pyrUp between them, a live frame's effect; the same again from the pending-call log; rtdd_refine_depth.
#include <cmath>

#include "pyramid.hpp"

namespace rtdd {

// src/main.cpp:249-259: the P - 1 coarse annotation levels and the coarsest level's injection, one launch (image_kernels.hip), for every
// image of the batch whatever the estimate covers: the flags are one per batch, the down-sampling only ever adds (an up-to-date image
// stays as it is) and a rebuild of an image that lost no label gives what it held.
static int annotation_pyramid(rtdd_ctx *ctx, Pyramid *p, bool rebuild) {
    const int P = p->levels;
    DeviceGuard g(ctx->device);
    uint8_t *sc[32], *ed[32]; size_t sp[32], ep[32], zs[32], ze[32]; int lr[32], lc[32];
    if (P > 12) return fail(ctx, RTDD_ERR_INVALID, "more than 12 pyramid levels");
    for (int l = 0; l < P; l++) {
        sc[l] = (uint8_t *)p->scribble[l].ptr; sp[l] = p->scribble[l].pitch; zs[l] = p->scribble[l].stride;
        ed[l] = (uint8_t *)p->edited[l].ptr; ep[l] = p->edited[l].pitch; ze[l] = p->edited[l].stride; lr[l] = p->edited[l].rows; lc[l] = p->edited[l].cols;
    }
    return launch_annotation_pyramid(ctx, P, sc, sp, zs, ed, ep, ze, lr, lc, (float *)p->depth[P - 1].ptr, p->depth[P - 1].pitch,
                                     p->depth[P - 1].stride, p->images, rebuild);
}

// the code planes of every level and every image of the batch from the level-0 region pair, one launch (cascade.hip)
static int region_codes(rtdd_ctx *ctx, Pyramid *p) {
    if (p->levels > RegionLevels::kMax) return fail(ctx, RTDD_ERR_INVALID, "more than 12 pyramid levels");
    DeviceGuard g(ctx->device);
    RegionLevels lv{};
    lv.n = p->levels;
    for (int l = 0; l < p->levels; l++) {
        const Image &im = p->region_code[l];
        lv.codes[l] = (uint8_t *)im.ptr; lv.pitch[l] = im.pitch; lv.stride[l] = im.stride; lv.rows[l] = im.rows; lv.cols[l] = im.cols; lv.shift[l] = l;
    }
    return launch_region_codes(ctx, (const uint8_t *)p->region_edited.ptr, p->region_edited.pitch, p->region_edited.stride,
                               (const uint8_t *)p->region_mask.ptr, p->region_mask.pitch, p->region_mask.stride, lv, p->images);
}
// in front of an estimate or a refinement: what the solves are to apply (0: nothing), the code planes brought up to date for it
static int regions_for_solve(rtdd_ctx *ctx, Pyramid *p, int *flags) {
    *flags = p->region_flags;
    if (p->region_flags == 0 || !p->regions_dirty) return RTDD_OK;
    // the planes are about to be rewritten, and a logged estimate that has to be run again reads them as they are: confirm (or heal)
    // what is logged first, while the codes it ran on still exist
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    RTDD_TRY(region_codes(ctx, p));
    p->regions_dirty = false;
    return RTDD_OK;
}

// Level l's solve on the pyramid's images from `first` on (t.batch.n of them in the same launches, blockIdx.z = image: Batch): the level's
// images, its guide -- gray[l], or level l of the colour chain -- and, with region flags, its codes, each with a batch's stride.
static SolveCall level_solve(const Pyramid *p, int first, int l, int guide, int regionFlags, const rtdd_solve_params &params, SolveTargets t) {
    const Image &gd = p->guide_image(guide, l);
    t.batch.first = first;
    t.batch.depth = p->depth[l].stride; t.batch.scribble = p->scribble[l].stride; t.batch.gray = gd.stride; t.batch.u8 = p->depth_u8.stride;
    SolveCall c{(float *)p->depth[l].at(first), p->depth[l].pitch, (const uint8_t *)p->scribble[l].at(first), p->scribble[l].pitch,
                (const uint8_t *)gd.at(first), gd.pitch, guide, p->depth[l].rows, p->depth[l].cols, l, params, t};
    if (regionFlags != 0) {
        const Image &rg = p->region_code[l];
        c.regions = (const uint8_t *)rg.at(first); c.regionsPitch = rg.pitch; c.regionFlags = regionFlags;
        c.targets.batch.regions = rg.stride;
    }
    return c;
}

// Levels from_level .. 0 of the estimate `e` (src/main.cpp:261-291); level_seq (optional) receives each level's solve sequence number.
static int estimate_levels(rtdd_ctx *ctx, const PendingOp::Estimate &e, int from_level, int *level_seq) {
    Pyramid *p = ctx->pyr;
    if (!p) return fail(ctx, RTDD_ERR_STATE, "the pyramid is gone");
    const int first = e.batch_first, n = e.batch_n;
    if (first < 0 || n < 1 || first + n > p->images) return fail(ctx, RTDD_ERR_INVALID, "images outside the pyramid's batch");
    const int P = p->levels;
    if (e.guide == RTDD_GUIDE_BGR && P > 1 && p->color.empty()) return fail(ctx, RTDD_ERR_STATE, "the colour guide's levels are gone");
    if (e.regionFlags != 0 && !p->has_regions()) return fail(ctx, RTDD_ERR_STATE, "the region codes are gone");
    if (from_level > P - 1) from_level = P - 1;
    int rc = RTDD_OK;
    for (int l = from_level; l >= 0 && rc == RTDD_OK; l--) {                   // src/main.cpp:261-288
        const int iters = (int)(e.maxIterations / powf(2.0, (P - 1) - l));     // :263
        const bool solved = p->depth[l].rows > 0 && p->depth[l].cols > 0;
        // Two launches less per level than the calls spelt out: above the finest level the solver's copy-back is left to the pyrUp
        // kernel (which reads the result plane directly and writes depth[l] on the side); at the finest level the copy-back also
        // writes the u8 map (:290).  Same values in the same buffers (tests/test_gpu_cascade.py compares every level's image).
        SolveTargets t;
        t.logged = false;                                                       // (the estimate is logged as one call)
        t.defer_finish = solved && l > 0;
        t.batch.n = n;
        if (l == 0) {
            t.u8 = (uint8_t *)p->depth_u8.at(first); t.u8_pitch = p->depth_u8.pitch;
            // (a live frame: its staging slot, or the host's buffer, too)
            t.u8b = e.live.u8; t.u8b_pitch = e.live.u8_pitch ? e.live.u8_pitch : p->depth_u8.pitch;
        }
        SolveOutcome done;
        if (solved) {
            // GPUMatrixFreeSolver(..., beta, CUDAIteration, CUDAThreshold, level): exactly `iters` sweeps (:266-268)
            const rtdd_solve_params sp{RTDD_METHOD_CHEBYSHEV_JACOBI, iters, /*tolerance=*/0.0f, /*checkEvery=*/0, /*relaxation=*/0.0f};
            rc = solve_with(ctx, level_solve(p, first, l, e.guide, e.regionFlags, sp, t), nullptr, &done);
            if (level_seq && l < 32) level_seq[l] = done.seq;
            if (rc == RTDD_OK) {
                p->level_info[l] = ctx->last_info; p->level_launch_images[l] = ctx->last_launch_images;
                if (ctx->last_info.kernel == 2) p->level_info[l].temporal_depth = ctx->last_nominal_depth;
            }
        }
        if (rc == RTDD_OK && l > 0) {
            DeviceGuard g(ctx->device);
            const Image &here = p->depth[l], &finer = p->depth[l - 1], &ed = p->edited[l - 1], &mk = p->scribble[l - 1];
            const float *src = (const float *)here.at(first); size_t sp = here.pitch;
            float *coarse_out = nullptr;
            PyrupBatch pb;
            pb.n = n; pb.src = here.stride; pb.dst = finer.stride; pb.edited = ed.stride; pb.mask = mk.stride; pb.coarse = here.stride;
            if (t.defer_finish) {                                               // the level's result is still in the solver's plane
                const size_t ip = plane_pitch(here.cols);
                const Level Lv = ctx->levels[l].view(first);
                src = Lv.P(done.plane, ip); sp = ip * sizeof(float); pb.src = Lv.elems * sizeof(float);
                coarse_out = (float *)here.at(first);
            }
            // guarded like k_finish (with the solve's sequence number): when level l's sweeps gave up it stores nothing, depth[l] keeps
            // level l's input and the level can be run again
            rc = launch_pyrup_inject(ctx, src, sp, here.rows, here.cols, (float *)finer.at(first), finer.pitch, finer.rows, finer.cols,
                                     (const uint8_t *)ed.at(first), ed.pitch, (const uint8_t *)mk.at(first), mk.pitch, coarse_out, here.pitch,
                                     /*guard_seq=*/solved ? done.seq : 0, &pb);     // :272-283
        }
    }
    if (rc != RTDD_OK) return rc;
    if (p->depth[0].rows > 0 && p->depth[0].cols > 0) return RTDD_OK;         // the u8 map left the solver's copy-back (above)
    DeviceGuard g(ctx->device);
    // (an image too small for a finest level: nothing above ran either)
    for (int b = first; b < first + n && rc == RTDD_OK; b++)
        rc = launch_depth_to_u8(ctx, (const float *)p->depth[0].at(b), p->depth[0].pitch, (uint8_t *)p->depth_u8.at(b), p->depth_u8.pitch,
                                p->rows, p->cols);   // :290
    return rc;
}

// A live frame's sticky effect (src/main.cpp:190-230) on the pyramid's level-0 images, into the frame's staging image (again, on a
// replay).  Queued on the compute stream right behind the estimate's copy-back: the f32 map it reads is still in the L2s / the
// Infinity Cache.
static int live_effect(rtdd_ctx *ctx, const LiveTargets &live) {
    Pyramid *p = ctx->pyr;
    if (!p) return fail(ctx, RTDD_ERR_STATE, "the pyramid is gone");
    if (p->rows <= 0 || p->cols <= 0 || !live.artistic) return RTDD_OK;
    DeviceGuard g(ctx->device);
    return launch_effect(ctx, {live.effect, (const uint8_t *)p->original.ptr, p->original.pitch, (const float *)p->depth[0].ptr, p->depth[0].pitch,
                               live.artistic, live.artistic_pitch, p->rows, p->cols, (const uint8_t *)p->gray[0].ptr, p->gray[0].pitch});
}

int estimate_submit(rtdd_ctx *ctx, int maxIterations, unsigned long long *op_id, bool whole_batch, const LiveTargets &live) {
    REQUIRE_PYRAMID(ctx);
    REQUIRE(ctx, maxIterations >= 0, "maxIterations must be >= 0");
    Pyramid *p = ctx->pyr;
    int annotation = PendingOp::kAnnotationNone;
    if (p->annotation_dirty) {
        RTDD_TRY(annotation_pyramid(ctx, p, p->annotation_rebuild));
        annotation = p->annotation_rebuild ? PendingOp::kAnnotationRebuilt : PendingOp::kAnnotationAccumulated;
        p->annotation_dirty = false; p->annotation_rebuild = false;
    }
    // the record the estimate runs from is the one it is logged as
    PendingOp op;
    op.kind = PendingOp::kEstimate; op.opt = ctx->opt;
    PendingOp::Estimate &e = op.estimate;
    e.annotation = annotation; e.maxIterations = maxIterations;
    e.batch_first = whole_batch ? 0 : p->sel; e.batch_n = whole_batch ? p->images : 1; e.live = live; e.guide = p->guide;
    RTDD_TRY(regions_for_solve(ctx, p, &e.regionFlags));
    int rc = estimate_levels(ctx, e, p->levels - 1, e.level_seq);
    if (rc == RTDD_OK && live.effect) rc = live_effect(ctx, live);      // src/main.cpp:190-230: the sticky effect, on this frame's map
    if (rc == RTDD_OK && log_call(ctx, op) && op_id) *op_id = op.id;
    return rc;
}

int estimate_replay(rtdd_ctx *ctx, const PendingOp::Estimate &e, int failed_seq) {
    Pyramid *p = ctx->pyr;
    if (!p) return fail(ctx, RTDD_ERR_STATE, "the pyramid is gone");
    int from = -1;                                  // the level whose solve gave up; an estimate queued behind the failed call: every level
    for (int l = 0; l < 32; l++) if (failed_seq != 0 && e.level_seq[l] == failed_seq) from = l;
    if (from < 0) for (int l = 31; l >= 0 && from < 0; l--) if (e.level_seq[l] != 0) from = l;
    // a live frame is run again on ITS annotation pair into ITS u8 slot and ITS artistic image (the newest frame's replay comes last: the
    // pyramid ends up naming its images)
    if (e.live.scribble) { p->scribble[0].ptr = e.live.scribble; p->edited[0].ptr = e.live.edited; }
    if (e.live.effect && e.live.artistic) p->artistic.ptr = e.live.artistic;
    // an estimate that rebuilt the coarse annotation levels rebuilds them again, from the pair set just above: a newer frame in flight
    // has added its strokes to them since.  The accumulating estimates run again behind it then add theirs again.
    if (e.annotation == PendingOp::kAnnotationRebuilt || (e.annotation == PendingOp::kAnnotationAccumulated && ctx->heal_rebuilt)) {
        RTDD_TRY(annotation_pyramid(ctx, p, e.annotation == PendingOp::kAnnotationRebuilt));
        ctx->heal_rebuilt = true;
    }
    int rc = from >= 0 ? estimate_levels(ctx, e, from, nullptr) : RTDD_OK;
    if (rc == RTDD_OK && e.live.effect) rc = live_effect(ctx, e.live);
    return rc;
}

}  // namespace rtdd

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

int rtdd_estimate_depth(rtdd_ctx *ctx, int maxIterations) { return estimate_submit(ctx, maxIterations, nullptr, /*whole_batch=*/false, LiveTargets()); }

int rtdd_estimate_depth_batch(rtdd_ctx *ctx, int maxIterations) { return estimate_submit(ctx, maxIterations, nullptr, /*whole_batch=*/true, LiveTargets()); }

int rtdd_refine_depth(rtdd_ctx *ctx, const rtdd_solve_params *params, rtdd_solve_info *info) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, params != nullptr, "null params");
    // the u8 map is written by the solve's own copy-back (k_finish: the same rounding as k_depth_to_u8), so that a solve that has to be
    // run again after a timed-out persistent launch brings the map with it
    SolveTargets t;
    t.u8 = (uint8_t *)p->depth_u8.at(p->sel); t.u8_pitch = p->depth_u8.pitch;
    int flags = 0;
    RTDD_TRY(regions_for_solve(ctx, p, &flags));
    return solve_with(ctx, level_solve(p, p->sel, 0, p->guide, flags, *params, t), info, nullptr);
}

}  // extern "C"
#pragma GCC visibility pop
