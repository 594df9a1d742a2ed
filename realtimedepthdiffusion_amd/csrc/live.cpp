// live.cpp -- live mode (rtdd_live_submit / rtdd_live_submit_ex / rtdd_live_wait): frames pipelined two deep over the estimate
// (estimate.cpp), their copies on streams of their own.
#include <cstring>
#include <new>

#include "pyramid.hpp"
#include "persist_sync.hpp"

namespace rtdd {

// Live mode (src/main.cpp:232-295, the body of the while loop, one frame): upload of the scribble and edited images (:236-237), the
// estimate, download of the u8 map (:290-291).  Frames are pipelined two deep: the copies run on a stream of their own, frame N+1's
// upload while frame N computes, frame N's download while frame N+1 computes.  Slot k = frame number % 2.
struct Live {
    // uploads and downloads each on a stream of their own: frame N+1's upload must not queue behind frame N's download
    hipStream_t up = nullptr, copy = nullptr;
    Image scribble_stage[2], edited_stage[2], u8_stage[2];
    hipEvent_t h2d_done[2] = {nullptr, nullptr}, est_done[2] = {nullptr, nullptr}, d2h_done[2] = {nullptr, nullptr};
    int *status_host = nullptr;           // page-locked, 2 x 8 ints: the kernels' control words as they were behind each frame's estimate
    // a frame's sticky depth effect (rtdd_live_submit_ex) renders here; allocated with the first such frame
    Image art_stage[2];
    // one host image a frame fills -- its u8 map, its artistic image -- and the staging image of the frame's slot it comes from
    struct Part { uint8_t *host = nullptr; size_t pitch = 0, width = 0; const Image *stage = nullptr; };
    struct Frame {
        Part map, art;
        bool direct = false;              // the copy-back kernel stores the map in the host's page-locked image itself
        unsigned long long op_id = 0;
        int effect = 0;                   // RTDD_EFFECT_*: the frame carries an artistic image too
        // its download was queued at submit on the compute stream (no other frame in flight); else rtdd_live_wait issues it
        bool art_queued = false;
    } frame[2];
    unsigned long long submitted = 0, waited = 0;
    // Round 5: no device-to-device staging copies.  A frame's annotation is uploaded into the staging pair that is NOT the pyramid's
    // current level-0 annotation, and the pyramid's level-0 scribble / edited images then simply BECOME that pair (pointer swap); the
    // frame's u8 map is written by the estimate's copy-back into RTDD_IMG_DEPTH_U8 AND into the frame's slot (k_finish: two targets).
    // The pyramid's own annotation buffers are kept here and put back before the pyramid is freed.
    void *own_scribble = nullptr, *own_edited = nullptr, *own_artistic = nullptr;
    Bounce bounce_art;                      // (an artistic image on its way to a host image with an unaligned pitch, compute stream)
    // ([frame parity][scribble, edited]: uploads of images with an unaligned host pitch, rtdd_live_submit)
    Bounce bounce_up[2][2];
    // page-locked: a staged map on its way to a host image with an unaligned pitch (live_fetch)
    uint8_t *host_bounce = nullptr; size_t host_bounce_bytes = 0;
};

// The device's name for a page-locked host image (every byte of rows x cols at `pitch` inside one registered range), or nullptr.  Asked
// for every frame (two driver queries, ~2 us of host time): a buffer freed and allocated again at the same address may not be page-locked
// any more.
static uint8_t *live_device_view(const uint8_t *host, size_t pitch, int rows, int cols) {
    uint8_t *dev = nullptr;
    hipPointerAttribute_t a0, a1;
    const uint8_t *last = host + (size_t)(rows - 1) * pitch + (size_t)cols - 1;
    if (hipPointerGetAttributes(&a0, host) == hipSuccess && hipPointerGetAttributes(&a1, last) == hipSuccess && a0.type == hipMemoryTypeHost
        && a1.type == hipMemoryTypeHost &&
        a0.devicePointer && a1.devicePointer && (const uint8_t *)a1.devicePointer - (const uint8_t *)a0.devicePointer == last - host)
        dev = (uint8_t *)a0.devicePointer;
    else (void)hipGetLastError();                                   // (an ordinary host pointer: the query fails, nothing else has)
    return dev;
}

bool live_stale_pointer(const Pyramid *p, const void *q) {
    const Live *v = p->live;
    if (!v || !q) return false;
    auto in_image = [](const void *base, const Image &like, const void *r) {
        return base && (const char *)r >= (const char *)base
            && (const char *)r < (const char *)base + like.pitch * (size_t)(like.rows > 0 ? like.rows : 1);
    };
    const void *olds[3] = {v->own_scribble, v->scribble_stage[0].ptr, v->scribble_stage[1].ptr};
    const void *olde[3] = {v->own_edited, v->edited_stage[0].ptr, v->edited_stage[1].ptr};
    for (int i = 0; i < 3; i++)
        if ((olds[i] != p->scribble[0].ptr && in_image(olds[i], p->scribble[0], q))
            || (olde[i] != p->edited[0].ptr && in_image(olde[i], p->edited[0], q)))
            return true;
    return false;
}

void live_free(Pyramid *p) {
    Live *v = p->live;
    if (!v) return;
    if (v->own_scribble) { p->scribble[0].ptr = v->own_scribble; p->edited[0].ptr = v->own_edited; }
    if (v->own_artistic) p->artistic.ptr = v->own_artistic;
    for (hipStream_t s : {v->up, v->copy}) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (int k = 0; k < 2; k++) {
        free_image(v->scribble_stage[k]); free_image(v->edited_stage[k]); free_image(v->u8_stage[k]); free_image(v->art_stage[k]);
        for (hipEvent_t e : {v->h2d_done[k], v->est_done[k], v->d2h_done[k]}) if (e) (void)hipEventDestroy(e);
    }
    if (v->status_host) (void)hipHostFree(v->status_host);
    for (auto &bb : v->bounce_up) for (Bounce &b : bb) if (b.ptr) (void)hipFree(b.ptr);
    if (v->host_bounce) (void)hipHostFree(v->host_bounce);
    if (v->bounce_art.ptr) (void)hipFree(v->bounce_art.ptr);
    delete v;
    p->live = nullptr;
}

static int live_create(rtdd_ctx *ctx) {
    Pyramid *p = ctx->pyr;
    if (p->live) return RTDD_OK;
    Live *v = new (std::nothrow) Live();
    if (!v) return fail(ctx, RTDD_ERR_NOMEM, "live state");
    p->live = v;
    // (never joins the null stream implicitly: the context's stream may be it)
    RTDD_HIP(ctx, hipStreamCreateWithFlags(&v->copy, hipStreamNonBlocking));
    RTDD_HIP(ctx, hipStreamCreateWithFlags(&v->up, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        RTDD_TRY(alloc_image(ctx, v->scribble_stage[k], p->rows, p->cols, 1, 0));
        RTDD_TRY(alloc_image(ctx, v->edited_stage[k], p->rows, p->cols, 3, 0));
        RTDD_TRY(alloc_image(ctx, v->u8_stage[k], p->rows, p->cols, 1, 0));
        for (hipEvent_t *e : {&v->h2d_done[k], &v->est_done[k], &v->d2h_done[k]}) RTDD_HIP(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    if (v->scribble_stage[0].pitch != p->scribble[0].pitch || v->edited_stage[0].pitch != p->edited[0].pitch || v->u8_stage[0].pitch != p->depth_u8.pitch)
        return fail(ctx, RTDD_ERR_STATE, "live staging images and pyramid images differ in pitch");
    v->own_scribble = p->scribble[0].ptr; v->own_edited = p->edited[0].ptr;
    RTDD_HIP(ctx, hipHostMalloc((void **)&v->status_host, 2 * 8 * sizeof(int), hipHostMallocDefault));
    for (int i = 0; i < 16; i++) v->status_host[i] = 0;
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));                                // the staging images' fills
    return RTDD_OK;
}

// Frame k's staged u8 map (`map`) and / or its artistic image (`art`), and the control words, to the host on the copy stream, and wait.
// A host image whose pitch is no multiple of four (slow_pitch): the staged image comes over WHOLE -- its rows, padding included, are one
// contiguous block -- into a page-locked buffer, one part behind the other, and the host copies the rows out; the runtime's 2-D copy
// takes 9 us per row for such a pitch, and a re-pitching kernel on the copy stream would queue behind the next frame's persistent
// launches (1921 x 1081: 1.39 ms per pipelined frame).
static int live_fetch(rtdd_ctx *ctx, Live *v, int k, bool map, bool art) {
    const int rows = ctx->pyr->rows;
    const Live::Frame &f = v->frame[k];
    struct { const Live::Part *q; bool bounced; size_t off; } parts[2] = {{map ? &f.map : nullptr, false, 0},
                                                                          {art && f.effect != 0 ? &f.art : nullptr, false, 0}};
    size_t bounce = 0;
    for (auto &s : parts)
        if (s.q && slow_pitch(s.q->pitch, rows)) { s.bounced = true; s.off = bounce; bounce += s.q->stage->pitch * (size_t)rows; }
    if (bounce > v->host_bounce_bytes) {
        if (v->host_bounce) {
            RTDD_HIP(ctx, hipStreamSynchronize(v->copy)); RTDD_HIP(ctx, hipHostFree(v->host_bounce));
            v->host_bounce = nullptr; v->host_bounce_bytes = 0;
        }
        RTDD_HIP(ctx, hipHostMalloc((void **)&v->host_bounce, bounce, hipHostMallocDefault));
        v->host_bounce_bytes = bounce;
    }
    for (const auto &s : parts) {
        if (!s.q) continue;
        const Image &st = *s.q->stage;
        if (s.bounced) RTDD_HIP(ctx, hipMemcpyAsync(v->host_bounce + s.off, st.ptr, st.pitch * (size_t)rows, hipMemcpyDeviceToHost, v->copy));
        else RTDD_HIP(ctx, hipMemcpy2DAsync(s.q->host, s.q->pitch, st.ptr, st.pitch, s.q->width, rows, hipMemcpyDeviceToHost, v->copy));
    }
    RTDD_HIP(ctx, hipMemcpyAsync(v->status_host + 8 * k, ctx->sync_words, 8 * sizeof(int), hipMemcpyDeviceToHost, v->copy));
    RTDD_HIP(ctx, hipStreamSynchronize(v->copy));
    for (const auto &s : parts)
        if (s.q && s.bounced)
            for (int y = 0; y < rows; y++)
                std::memcpy(s.q->host + (size_t)y * s.q->pitch, v->host_bounce + s.off + (size_t)y * s.q->stage->pitch, s.q->width);
    return RTDD_OK;
}

}  // namespace rtdd

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

int rtdd_live_pending(rtdd_ctx *ctx) {
    if (!ctx || !ctx->pyr || !ctx->pyr->live) return 0;
    return (int)(ctx->pyr->live->submitted - ctx->pyr->live->waited);
}

int rtdd_live_wait(rtdd_ctx *ctx) {
    if (!ctx) return RTDD_ERR_INVALID;
    if (rtdd_live_pending(ctx) == 0) return fail(ctx, RTDD_ERR_STATE, "no frame in flight");
    Live *v = ctx->pyr->live;
    DeviceGuard g(ctx->device);
    const int k = (int)(v->waited % 2);
    const Live::Frame &fr = v->frame[k];
    const bool fetch_map = !fr.direct, fetch_art = fr.effect != 0 && !fr.art_queued;
    if (!fetch_map && !fetch_art) RTDD_HIP(ctx, hipEventSynchronize(v->d2h_done[k]));
    else {
        // (a frame with one part stored / queued on the compute stream and the other staged: the one event behind both was recorded there)
        RTDD_HIP(ctx, hipEventSynchronize(fr.direct ? v->d2h_done[k] : v->est_done[k]));
        RTDD_TRY(live_fetch(ctx, v, k, fetch_map, fetch_art));
    }
    // the usual case: the frame is good, and so is everything logged before it
    if (v->status_host[8 * k + kSyncStatus] == 0) {
        size_t n = 0;
        while (n < ctx->pending.size() && ctx->pending[n].id <= v->frame[k].op_id) n++;
        ctx->pending.erase(ctx->pending.begin(), ctx->pending.begin() + n);
        v->waited++;
        return RTDD_OK;
    }
    // A sweep launch in front of this frame's download gave up (include/rtdd.h, RTDD_ERR_TIMEOUT): drain both streams, let the
    // status check run the logged estimates again (each brings its staged u8 map and its effect with it), then fetch every frame in
    // flight again.
    RTDD_HIP(ctx, hipStreamSynchronize(v->up));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(v->copy));
    note_status_writer(ctx);
    RTDD_TRY(check_persistent_status(ctx));
    for (unsigned long long f = v->waited; f < v->submitted; f++) {
        const int j = (int)(f % 2);
        // (a frame whose map the copy-back kernel stores in the host's buffer itself has just been run again into that buffer; an
        // artistic image is always rendered into its staging slot)
        RTDD_TRY(live_fetch(ctx, v, j, !v->frame[j].direct, true));
        v->status_host[8 * j + kSyncStatus] = 0;
    }
    v->waited++;
    return RTDD_OK;
}

int rtdd_live_submit(rtdd_ctx *ctx, const uint8_t *hostScribble, size_t scribblePitch, const uint8_t *hostEdited, size_t editedPitch,
                     int maxIterations, uint8_t *hostDepthU8, size_t depthPitch) {
    return rtdd_live_submit_ex(ctx, hostScribble, scribblePitch, hostEdited, editedPitch, maxIterations, hostDepthU8, depthPitch, RTDD_EFFECT_NONE, nullptr, 0);
}

int rtdd_live_submit_ex(rtdd_ctx *ctx, const uint8_t *hostScribble, size_t scribblePitch, const uint8_t *hostEdited, size_t editedPitch,
                        int maxIterations, uint8_t *hostDepthU8, size_t depthPitch, int effect, uint8_t *hostArtistic, size_t artisticPitch) {
    REQUIRE_PYRAMID(ctx);
    Pyramid *p = ctx->pyr;
    REQUIRE(ctx, (hostScribble == nullptr) == (hostEdited == nullptr), "scribble and edited images come together (or neither: the annotation is unchanged)");
    REQUIRE(ctx, !hostScribble || (scribblePitch >= (size_t)p->cols && editedPitch >= (size_t)p->cols * 3), "pitch smaller than a row");
    REQUIRE(ctx, hostDepthU8 && depthPitch >= (size_t)p->cols && maxIterations >= 0, "bad output buffer or iteration count");
    REQUIRE(ctx, effect >= RTDD_EFFECT_NONE && effect <= RTDD_EFFECT_HAZE, "unknown effect");
    REQUIRE(ctx, effect == RTDD_EFFECT_NONE || (hostArtistic && artisticPitch >= (size_t)p->cols * 3), "an effect needs a host image for its result");
    REQUIRE(ctx, p->images == 1, "live frames run on a single-image pyramid (rtdd_pyramid_create)");
    DeviceGuard g(ctx->device);
    RTDD_TRY(live_create(ctx));
    Live *v = p->live;
    // two frames in flight at most: the slot is free again
    if (v->submitted - v->waited >= 2) RTDD_TRY(rtdd_live_wait(ctx));
    const int k = (int)(v->submitted % 2);
    const bool lone = v->submitted == v->waited;          // no other frame in flight: nothing for a copy to overlap
    if (effect != RTDD_EFFECT_NONE && !v->art_stage[0].ptr) {          // the first frame with an effect: its two staging images
        for (int j = 0; j < 2; j++) RTDD_TRY(alloc_image(ctx, v->art_stage[j], p->rows, p->cols, 3, 0));
        if (v->art_stage[0].pitch != p->artistic.pitch) return fail(ctx, RTDD_ERR_STATE, "live staging images and pyramid images differ in pitch");
        v->own_artistic = p->artistic.ptr;
    }
    if (hostScribble) {
        // upload into the staging pair the pyramid is NOT looking at: the only frame that can still be in flight reads the other one
        // (at most two frames in flight, and the older one has been waited for above)
        const int u = p->scribble[0].ptr == v->scribble_stage[0].ptr ? 1 : 0;
        // (no other frame in flight: the upload goes on the compute stream itself, no event between the streams: 1080p 1.335 -> 1.324 ms
        // one frame at a time, 4K 2.21 -> 2.18)
        hipStream_t us = lone ? ctx->stream : v->up;
        // The two halves of copy_h2d around the upload's event.  A host image whose pitch is no multiple of four goes as one linear copy
        // into a contiguous buffer of this frame's parity on the upload stream, and is re-pitched into the staging image by a kernel on
        // the COMPUTE stream, behind the upload's event: on the upload stream that kernel would queue behind the running frame's
        // persistent launches.  (The buffer is written again two frames later, after this frame has been waited for.)
        const struct { const uint8_t *host; size_t hp, width; const Image &dst; Bounce &b; } ups[2] = {
            {hostScribble, scribblePitch, (size_t)p->cols, v->scribble_stage[u], v->bounce_up[k][0]},
            {hostEdited, editedPitch, (size_t)p->cols * 3, v->edited_stage[u], v->bounce_up[k][1]}};
        for (auto &q : ups) RTDD_TRY(copy_h2d_linear(ctx, q.b, q.dst.ptr, q.dst.pitch, q.host, q.hp, q.width, p->rows, us, ctx->stream));
        if (!lone) {
            RTDD_HIP(ctx, hipEventRecord(v->h2d_done[k], v->up));
            RTDD_HIP(ctx, hipStreamWaitEvent(ctx->stream, v->h2d_done[k], 0));
        }
        for (auto &q : ups) RTDD_TRY(copy_h2d_repitch(ctx, q.b, q.dst.ptr, q.dst.pitch, q.hp, q.width, p->rows, ctx->stream));
        // the pyramid's level-0 annotation IS the uploaded pair: no copy
        p->scribble[0].ptr = v->scribble_stage[u].ptr; p->edited[0].ptr = v->edited_stage[u].ptr;
        p->annotation_dirty = true;
    }
    unsigned long long op_id = ctx->op_counter;
    // Where the map goes.  What it must not do is make a copy stream wait for the compute stream ON THE DEVICE: that costs the compute
    // stream ~80 us per frame on this runtime (with both copies removed and only the event pair left: still 80; EXPERIMENTS.md round 5).
    //   * another frame in flight (a pipelined loop): the map goes to the frame's staging slot, and rtdd_live_wait -- the HOST, which is
    //     idle for 0.9 of such a frame -- downloads it once the estimate's event has come; the copy overlaps the next frame's arithmetic
    //     (1080p 1.21 -> 1.14 ms per frame, 4K 1.57 -> 1.52);
    //   * no other frame in flight (one frame at a time: nothing could overlap a download) and a page-locked host buffer (rtdd_host_alloc,
    //     hipHostMalloc, hipHostRegister: device-visible): the estimate's copy-back kernel stores the u8 map straight into it, ~20 us
    //     per MB of posted writes, and the frame ends with an event on the compute stream (1080p 1.42 -> 1.33 ms, 4K 2.31 -> 2.20).
    // The artistic image of a frame with an effect (6.2 MB at 1080p) is rendered into the frame's staging slot and follows the same
    // rule: downloaded by rtdd_live_wait from the host when pipelined, queued behind the effect on the compute stream when alone.
    const bool want_direct = ctx->opt.live_zero_copy == 2 || (ctx->opt.live_zero_copy == 1 && lone);
    uint8_t *direct = want_direct ? live_device_view(hostDepthU8, depthPitch, p->rows, p->cols) : nullptr;
    const Live::Part map{hostDepthU8, depthPitch, (size_t)p->cols, &v->u8_stage[k]};
    const Live::Part art{hostArtistic, artisticPitch, (size_t)p->cols * 3, &v->art_stage[k]};
    // (the estimate's copy-back writes this frame's map into RTDD_IMG_DEPTH_U8 and into the frame's second target: estimate_levels)
    LiveTargets lt;
    lt.scribble = p->scribble[0].ptr; lt.edited = p->edited[0].ptr;
    lt.u8 = direct ? direct : (uint8_t *)map.stage->ptr; lt.u8_pitch = direct ? depthPitch : 0;
    lt.effect = effect;
    if (effect != RTDD_EFFECT_NONE) {
        lt.artistic = (uint8_t *)art.stage->ptr; lt.artistic_pitch = art.stage->pitch;
        // RTDD_IMG_ARTISTIC names the newest frame's image (like the annotation pair: no copy)
        p->artistic.ptr = art.stage->ptr;
    }
    RTDD_TRY(estimate_submit(ctx, maxIterations, &op_id, /*whole_batch=*/false, lt));
    const bool art_queued = effect != RTDD_EFFECT_NONE && lone;
    if (art_queued) RTDD_TRY(copy_d2h(ctx, v->bounce_art, art.host, art.pitch, art.stage->ptr, art.stage->pitch, art.width, p->rows, ctx->stream));
    if (direct) {
        RTDD_HIP(ctx, hipMemcpyAsync(v->status_host + 8 * k, ctx->sync_words, 8 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        RTDD_HIP(ctx, hipEventRecord(v->d2h_done[k], ctx->stream));
    } else {
        // staged: the download is issued by rtdd_live_wait, from the HOST, once this event has come -- a copy stream made to wait for the
        // compute stream on the device costs the compute stream ~80 us per frame (above); the host has the time (it is idle for 0.9 of a
        // pipelined frame), and the copy still overlaps the next frame's arithmetic
        RTDD_HIP(ctx, hipEventRecord(v->est_done[k], ctx->stream));
    }
    Live::Frame &fr = v->frame[k];
    fr.map = map; fr.art = art; fr.op_id = op_id; fr.direct = direct != nullptr; fr.effect = effect; fr.art_queued = art_queued;
    v->submitted++;
    return RTDD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
