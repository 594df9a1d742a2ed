// effects_api.cpp -- the rtdd_simulate_* entry points (include/rtdd.h): arguments checked, one Effect record built, handed to
// launch_effect (effect_kernels.hip) and, behind unconfirmed solves, to the pending-call log (heal.cpp).  Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rtdd_internal.hpp"

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

static int check_effect(rtdd_ctx *ctx, const void *a, const void *b, const void *c, size_t op, size_t dp, size_t ap, int rows, int cols) {
    REQUIRE(ctx, a && b && c, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    REQUIRE(ctx, (long long)rows * rows + (long long)cols * cols < 2147483647LL, "image too large");
    REQUIRE(ctx, op >= (size_t)cols * 3 && ap >= (size_t)cols * 3 && dp >= (size_t)cols * 4, "pitch smaller than a row");
    REQUIRE(ctx, f32_image_aligned(b, dp), kF32AlignText);         // (b: the depth map)
    return RTDD_OK;
}

// What every rtdd_simulate_* does once its arguments are checked: launch, and log the effect if it sits behind unconfirmed solves.
static int simulate(rtdd_ctx *ctx, const Effect &e) {
    DeviceGuard g(ctx->device);
    RTDD_TRY(launch_effect(ctx, e));
    PendingOp op;
    op.kind = PendingOp::kEffect; op.opt = ctx->opt; op.effect = e;
    log_call(ctx, op);
    return RTDD_OK;
}

int rtdd_simulate_defocus(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                          uint8_t *artistic, size_t artisticPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK || rows == 0 || cols == 0) return rc;
    REQUIRE(ctx, original != artistic, "defocus cannot run in place");
    return simulate(ctx, {RTDD_EFFECT_DEFOCUS, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols});
}

int rtdd_simulate_desaturation(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const uint8_t *gray, size_t grayPitch,
                               const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK || rows == 0 || cols == 0) return rc;
    REQUIRE(ctx, gray && grayPitch >= (size_t)cols, "bad gray image");
    return simulate(ctx, {RTDD_EFFECT_DESATURATION, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols, gray,
                          grayPitch});
}

int rtdd_simulate_haze(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                       uint8_t *artistic, size_t artisticPitch, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK || rows == 0 || cols == 0) return rc;
    return simulate(ctx, {RTDD_EFFECT_HAZE, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols});
}

// the aperture (the K rule) and the focus of rtdd_simulate_refocus, rtdd_simulate_lens_blur and rtdd_simulate_bokeh
static int check_focus(rtdd_ctx *ctx, int rows, int cols, double aperture, float focusDepth, int focusX, int focusY) {
    REQUIRE(ctx, std::isfinite(aperture) && aperture >= 0.0, "aperture must be finite and >= 0");
    REQUIRE(ctx, window_scale(aperture, rows, cols) <= 255, "aperture too large: the window scale (int)(aperture * diagonal) must be <= 255");
    if (focusX < 0) REQUIRE(ctx, std::isfinite(focusDepth), "focusDepth must be finite");
    else REQUIRE(ctx, focusX < cols && focusY >= 0 && focusY < rows, "focus pixel outside the image");
    return RTDD_OK;
}

int rtdd_simulate_refocus(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                          uint8_t *artistic, size_t artisticPitch, int rows, int cols, double aperture, float focusDepth, int focusX, int focusY) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    rc = check_focus(ctx, rows, cols, aperture, focusDepth, focusX, focusY);
    if (rc != RTDD_OK) return rc;
    const int kernelSize = window_scale(aperture, rows, cols);
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "refocus cannot run in place");
    Effect e{Effect::kRefocus, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    e.kernelSize = kernelSize; e.focusDepth = focusDepth; e.focusX = focusX; e.focusY = focusY;
    return simulate(ctx, e);
}

int rtdd_simulate_lens_blur(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                            uint8_t *artistic, size_t artisticPitch, int rows, int cols, double aperture, float focusDepth, int focusX, int focusY,
                            int shape) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, shape == RTDD_APERTURE_BOX || shape == RTDD_APERTURE_DISC, "shape must be RTDD_APERTURE_BOX or RTDD_APERTURE_DISC");
    // the square aperture IS a refocus: the same checks, the same Effect, the same kernels
    if (shape == RTDD_APERTURE_BOX)
        return rtdd_simulate_refocus(ctx, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols, aperture, focusDepth, focusX, focusY);
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    rc = check_focus(ctx, rows, cols, aperture, focusDepth, focusX, focusY);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, original != artistic, "lens blur cannot run in place");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kLensBlur, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    e.kernelSize = window_scale(aperture, rows, cols); e.focusDepth = focusDepth; e.focusX = focusX; e.focusY = focusY;
    return simulate(ctx, e);
}

int rtdd_simulate_bokeh(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                        uint8_t *artistic, size_t artisticPitch, int rows, int cols, double aperture, float focusDepth, int focusX, int focusY) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    rc = check_focus(ctx, rows, cols, aperture, focusDepth, focusX, focusY);
    if (rc != RTDD_OK) return rc;
    const int kernelSize = window_scale(aperture, rows, cols);
    REQUIRE(ctx, kernelSize <= 127, "aperture too large for the bokeh: the window scale (int)(aperture * diagonal) must be <= 127");
    REQUIRE(ctx, original != artistic, "bokeh cannot run in place");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kBokeh, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    e.kernelSize = kernelSize; e.focusDepth = focusDepth; e.focusX = focusX; e.focusY = focusY;
    return simulate(ctx, e);
}

int rtdd_simulate_haze_ex(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                          uint8_t *artistic, size_t artisticPitch, int rows, int cols, float beta, uint8_t airB, uint8_t airG, uint8_t airR) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, std::isfinite(beta) && beta >= 0.0f && beta <= 64.0f, "beta must be finite and in [0, 64]");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kHazeEx, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    e.beta = beta; e.air = (uint32_t)airB | ((uint32_t)airG << 8) | ((uint32_t)airR << 16);
    return simulate(ctx, e);
}

int rtdd_simulate_stereo(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                         uint8_t *artistic, size_t artisticPitch, int rows, int cols, int disparity, float zeroParallaxDepth, int zeroX, int zeroY,
                         int mode) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, disparity >= -256 && disparity <= 256, "|disparity| must be <= 256");
    REQUIRE(ctx, mode == RTDD_STEREO_VIEW || mode == RTDD_STEREO_ANAGLYPH, "mode must be RTDD_STEREO_VIEW or RTDD_STEREO_ANAGLYPH");
    if (zeroX < 0) REQUIRE(ctx, std::isfinite(zeroParallaxDepth) && zeroParallaxDepth >= 0.0f && zeroParallaxDepth <= 255.0f,
                           "zeroParallaxDepth must be finite and in [0, 255]");
    else REQUIRE(ctx, zeroX < cols && zeroY >= 0 && zeroY < rows, "zero-parallax pixel outside the image");
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "stereo cannot run in place");
    Effect e{Effect::kStereo, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    e.disparity = disparity; e.zeroDepth = zeroParallaxDepth; e.zeroX = zeroX; e.zeroY = zeroY; e.stereoMode = mode;
    return simulate(ctx, e);
}

// The checks of rtdd_simulate_relight up to the empty image, and the light as the kernels take it (e.light), for the two relight calls.
static int prepare_relight(rtdd_ctx *ctx, Effect &e, const rtdd_light *light) {
    const int rows = e.rows, cols = e.cols;
    int rc = check_effect(ctx, e.original, e.depth, e.artistic, e.originalPitch, e.depthPitch, e.artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, light, "null light");
    const rtdd_light &q = *light;
    const bool point = q.kind == RTDD_LIGHT_POINT;
    REQUIRE(ctx, point || q.kind == RTDD_LIGHT_DIRECTIONAL, "kind must be RTDD_LIGHT_DIRECTIONAL or RTDD_LIGHT_POINT");
    for (float v : {q.x, q.y, q.z, q.anchorDepth, q.radius, q.relief, q.ambient, q.diffuse}) REQUIRE(ctx, std::isfinite(v), "a non-finite value in the light");
    REQUIRE(ctx, q.z > 0.0f, "the light's z must be > 0");
    REQUIRE(ctx, q.relief >= 0.0f && q.relief <= 64.0f, "relief outside [0, 64]");
    REQUIRE(ctx, q.ambient >= 0.0f && q.ambient <= 8.0f && q.diffuse >= 0.0f && q.diffuse <= 8.0f, "ambient or diffuse outside [0, 8]");
    Effect::Light &L = e.light;
    L.kind = q.kind;
    if (point) {
        REQUIRE(ctx, q.x >= -32768.0f && q.x <= 32767.0f && q.y >= -32768.0f && q.y <= 32767.0f, "a point light's x or y outside [-32768, 32767]");
        REQUIRE(ctx, q.z <= 65536.0f, "a point light's z above 65536");
        REQUIRE(ctx, q.radius > 0.0f && q.radius <= 65536.0f, "radius outside (0, 65536]");
        if (q.anchorX < 0) REQUIRE(ctx, q.anchorDepth >= 0.0f && q.anchorDepth <= 255.0f, "anchorDepth outside [0, 255]");
        else REQUIRE(ctx, q.anchorX < cols && q.anchorY >= 0 && q.anchorY < rows, "anchor pixel outside the image");
        L.x = q.x; L.y = q.y; L.z = q.z;
        L.anchorDepth = q.anchorDepth; L.anchorX = q.anchorX; L.anchorY = q.anchorY;
        L.invR2 = (float)(1.0 / ((double)q.radius * q.radius));
    } else {
        const double len = std::sqrt((((double)q.x * q.x) + ((double)q.y * q.y)) + ((double)q.z * q.z));
        REQUIRE(ctx, std::isfinite(len) && len > 0.0, "the light's direction has no length");
        L.x = (float)(q.x / len); L.y = (float)(q.y / len); L.z = (float)(q.z / len);
    }
    L.relief = q.relief; L.ambient = q.ambient;
    const uint8_t color[3] = {q.colorB, q.colorG, q.colorR};
    for (int c = 0; c < 3; c++) L.k[c] = (float)((double)q.diffuse * color[c] / 255.0);
    return RTDD_OK;
}

int rtdd_simulate_relight(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                          uint8_t *artistic, size_t artisticPitch, int rows, int cols, const rtdd_light *light) {
    if (!ctx) return RTDD_ERR_INVALID;
    Effect e{Effect::kRelight, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    const int rc = prepare_relight(ctx, e, light);
    if (rc != RTDD_OK) return rc;
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "relight cannot run in place");
    return simulate(ctx, e);
}

// The checks of rtdd_simulate_relight_shadowed's shadow, and the march as the kernels take it (e.shadow); e.light is prepared.
static int prepare_shadow(rtdd_ctx *ctx, Effect &e, const rtdd_shadow *shadow) {
    REQUIRE(ctx, shadow, "null shadow");
    const rtdd_shadow &q = *shadow;
    for (float v : {q.bias, q.softness, q.strength}) REQUIRE(ctx, std::isfinite(v), "a non-finite value in the shadow");
    REQUIRE(ctx, q.maxSteps >= 0 && q.maxSteps <= 1024, "maxSteps outside [0, 1024]");
    REQUIRE(ctx, q.bias >= 0.0f && q.bias <= 65536.0f && q.softness >= 0.0f && q.softness <= 65536.0f, "bias or softness outside [0, 65536]");
    REQUIRE(ctx, q.strength >= 0.0f && q.strength <= 1.0f, "strength outside [0, 1]");
    Effect::Shadow &S = e.shadow;
    S.maxSteps = q.maxSteps; S.bias = q.bias; S.softness = q.softness; S.strength = q.strength;
    if (e.light.kind == RTDD_LIGHT_DIRECTIONAL) {
        // the step along the major axis of the projected direction, in f32; m == 0 (the light straight above) leaves sx == sy == 0
        const float m = fmaxf(fabsf(e.light.x), fabsf(e.light.y));
        if (m != 0.0f) { S.sx = e.light.x / m; S.sy = e.light.y / m; S.rise = e.light.z / m; }
    }
    return RTDD_OK;
}

int rtdd_simulate_relight_shadowed(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                                   uint8_t *artistic, size_t artisticPitch, int rows, int cols, const rtdd_light *light,
                                   const rtdd_shadow *shadow) {
    if (!ctx) return RTDD_ERR_INVALID;
    Effect e{Effect::kRelightShadow, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    int rc = prepare_relight(ctx, e, light);
    if (rc != RTDD_OK) return rc;
    rc = prepare_shadow(ctx, e, shadow);
    if (rc != RTDD_OK) return rc;
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "relight cannot run in place");
    return simulate(ctx, e);
}

// The checks of rtdd_simulate_parallax's view behind the images', and the view as the kernels take it (e.parallax), for the two parallax calls.
static int prepare_parallax(rtdd_ctx *ctx, Effect &e, const rtdd_parallax *view) {
    const int rows = e.rows, cols = e.cols;
    REQUIRE(ctx, view, "null view");
    const rtdd_parallax &q = *view;
    REQUIRE(ctx, q.shiftX >= -256 && q.shiftX <= 256 && q.shiftY >= -256 && q.shiftY <= 256, "|shiftX| and |shiftY| must be <= 256");
    const int span = std::max(std::max(cols - 1, rows - 1), 0);
    REQUIRE(ctx, std::isfinite(q.dolly) && std::fabs((double)q.dolly) * span / 2.0 <= 256.0,
            "dolly must be finite with |dolly| * max(cols - 1, rows - 1) / 2 <= 256");
    if (q.zeroX < 0) REQUIRE(ctx, std::isfinite(q.zeroParallaxDepth) && q.zeroParallaxDepth >= 0.0f && q.zeroParallaxDepth <= 255.0f,
                             "zeroParallaxDepth must be finite and in [0, 255]");
    else REQUIRE(ctx, q.zeroX < cols && q.zeroY >= 0 && q.zeroY < rows, "zero-parallax pixel outside the image");
    Effect::Parallax &P = e.parallax;
    P.shiftX = q.shiftX; P.shiftY = q.shiftY; P.dolly = q.dolly; P.zeroX = q.zeroX; P.zeroY = q.zeroY;
    P.zeroDepth = q.zeroParallaxDepth;
    P.cx = (float)(cols - 1) * 0.5f; P.cy = (float)(rows - 1) * 0.5f;
    return RTDD_OK;
}

int rtdd_simulate_parallax(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                           uint8_t *artistic, size_t artisticPitch, int rows, int cols, const rtdd_parallax *view) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    Effect e{Effect::kParallax, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    rc = prepare_parallax(ctx, e, view);
    if (rc != RTDD_OK) return rc;
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "parallax cannot run in place");
    return simulate(ctx, e);
}

int rtdd_simulate_parallax_layered(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                                   const uint8_t *plate, size_t platePitch, const float *plateDepth, size_t plateDepthPitch,
                                   uint8_t *artistic, size_t artisticPitch, float *depthOut, size_t depthOutPitch, uint8_t *coverage,
                                   size_t coveragePitch, int rows, int cols, const rtdd_parallax *view) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, (plate == nullptr) == (plateDepth == nullptr), "plate and plateDepth must both be given or both be null");
    if (plate) {
        REQUIRE(ctx, platePitch >= (size_t)cols * 3 && plateDepthPitch >= (size_t)cols * 4, "pitch smaller than a row");
        REQUIRE(ctx, f32_image_aligned(plateDepth, plateDepthPitch), kF32AlignText);
    }
    if (depthOut) {
        REQUIRE(ctx, depthOutPitch >= (size_t)cols * 4, "pitch smaller than a row");
        REQUIRE(ctx, f32_image_aligned(depthOut, depthOutPitch), kF32AlignText);
    }
    if (coverage) REQUIRE(ctx, coveragePitch >= (size_t)cols, "pitch smaller than a row");
    Effect e{Effect::kParallaxLayered, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    rc = prepare_parallax(ctx, e, view);
    if (rc != RTDD_OK) return rc;
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic && plate != artistic, "parallax cannot run in place");
    REQUIRE(ctx, !depthOut || ((const float *)depthOut != depth && (const float *)depthOut != plateDepth), "parallax cannot run in place");
    Effect::ParallaxLayers &l = e.layers;
    if (plate) { l.plate = plate; l.platePitch = platePitch; l.plateDepth = plateDepth; l.plateDepthPitch = plateDepthPitch; }
    if (depthOut) { l.depthOut = depthOut; l.depthOutPitch = depthOutPitch; }
    if (coverage) { l.coverage = coverage; l.coveragePitch = coveragePitch; }
    return simulate(ctx, e);
}

// The checks of rtdd_simulate_ambient_occlusion behind the images', and the occlusion and the light as the kernels take them
// (e.occlusion, e.light): the occlusion first; then the light, checked as rtdd_simulate_relight checks it.
static int prepare_occlusion(rtdd_ctx *ctx, Effect &e, const rtdd_ambient_occlusion *ao, const rtdd_light *light) {
    REQUIRE(ctx, ao, "null ao");
    const rtdd_ambient_occlusion &q = *ao;
    REQUIRE(ctx, q.mode == RTDD_AO_SHADE || q.mode == RTDD_AO_MAP, "mode must be RTDD_AO_SHADE or RTDD_AO_MAP");
    REQUIRE(ctx, q.directions == 4 || q.directions == 8, "directions must be 4 or 8");
    REQUIRE(ctx, q.radius >= 0 && q.radius <= 64, "radius outside [0, 64]");
    for (float v : {q.relief, q.bias, q.strength}) REQUIRE(ctx, std::isfinite(v), "a non-finite value in the ambient occlusion");
    REQUIRE(ctx, q.relief >= 0.0f && q.relief <= 64.0f, "relief outside [0, 64]");
    REQUIRE(ctx, q.bias >= 0.0f && q.bias <= 65536.0f, "bias outside [0, 65536]");
    REQUIRE(ctx, q.strength >= 0.0f && q.strength <= 1.0f, "strength outside [0, 1]");
    Effect::Occlusion &A = e.occlusion;
    A.mode = q.mode; A.directions = q.directions; A.radius = q.radius; A.relief = q.relief; A.bias = q.bias; A.strength = q.strength;
    A.lit = light != nullptr;
    if (light) {
        REQUIRE(ctx, q.mode != RTDD_AO_MAP, "RTDD_AO_MAP takes no light");
        const int rc = prepare_relight(ctx, e, light);
        if (rc != RTDD_OK) return rc;
        REQUIRE(ctx, std::memcmp(&q.relief, &light->relief, sizeof(float)) == 0, "ao->relief must equal light->relief bit for bit");
    }
    return RTDD_OK;
}

int rtdd_simulate_ambient_occlusion(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                                    uint8_t *artistic, size_t artisticPitch, int rows, int cols, const rtdd_ambient_occlusion *ao,
                                    const rtdd_light *light) {
    if (!ctx) return RTDD_ERR_INVALID;
    Effect e{Effect::kAmbientOcclusion, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    // the images first, as every effect
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    rc = prepare_occlusion(ctx, e, ao, light);
    if (rc != RTDD_OK) return rc;
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "ambient occlusion cannot run in place");
    return simulate(ctx, e);
}

int rtdd_simulate_lighting(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                           uint8_t *artistic, size_t artisticPitch, int rows, int cols, const rtdd_light *light, const rtdd_shadow *shadow,
                           const rtdd_ambient_occlusion *ao) {
    if (!ctx) return RTDD_ERR_INVALID;
    Effect e{Effect::kLighting, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    // the checks of the two calls it fuses, each by its own function: the images and the light, the shadow, the occlusion under that light
    int rc = prepare_relight(ctx, e, light);
    if (rc != RTDD_OK) return rc;
    rc = prepare_shadow(ctx, e, shadow);
    if (rc != RTDD_OK) return rc;
    rc = prepare_occlusion(ctx, e, ao, light);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, ao->mode == RTDD_AO_SHADE, "lighting takes RTDD_AO_SHADE only");
    if (rows == 0 || cols == 0) return RTDD_OK;
    REQUIRE(ctx, original != artistic, "lighting cannot run in place");
    return simulate(ctx, e);
}

// How many pixels p = origin, origin + 1, ... a sprite axis of `texels` texels covers (include/rtdd.h rtdd_composite_layer, step 1):
// those with (2 (p - origin) + 1) * 32768 < 256 * texels * scale, i.e. 2 (p - origin) + 1 < texels * scale / 128.
static int layer_extent(int texels, int scale) { return (texels * scale + 127) / 256; }        // (texels * scale <= 2^26)

int rtdd_composite_layer(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                         const uint8_t *sprite, size_t spritePitch, uint8_t *artistic, size_t artisticPitch, float *depthOut,
                         size_t depthOutPitch, int rows, int cols, const rtdd_layer *layer) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    if (depthOut) {
        REQUIRE(ctx, depthOutPitch >= (size_t)cols * 4, "pitch smaller than a row");
        REQUIRE(ctx, f32_image_aligned(depthOut, depthOutPitch), kF32AlignText);
    }
    REQUIRE(ctx, original != artistic && (const float *)depthOut != depth, "a layer cannot be composited in place");
    REQUIRE(ctx, layer, "null layer");
    const rtdd_layer &q = *layer;
    REQUIRE(ctx, q.rows >= 1 && q.rows <= 16384 && q.cols >= 1 && q.cols <= 16384, "the sprite's rows or cols outside [1, 16384]");
    REQUIRE(ctx, sprite && spritePitch >= (size_t)q.cols * 4, "bad sprite image");
    for (int v : {q.x, q.y, q.x0, q.y0, q.x1, q.y1}) REQUIRE(ctx, v >= -16384 && v <= 16383, "a layer coordinate outside [-16384, 16383]");
    REQUIRE(ctx, q.scale >= 16 && q.scale <= 4096, "scale outside [16, 4096]");
    REQUIRE(ctx, q.filter == RTDD_LAYER_NEAREST || q.filter == RTDD_LAYER_BILINEAR, "filter must be RTDD_LAYER_NEAREST or RTDD_LAYER_BILINEAR");
    REQUIRE(ctx, q.opacity >= 0 && q.opacity <= 255, "opacity outside [0, 255]");
    for (float v : {q.depth0, q.depth1, q.feather}) REQUIRE(ctx, std::isfinite(v), "a non-finite value in the layer");
    REQUIRE(ctx, q.depth0 >= 0.0f && q.depth0 <= 255.0f && q.depth1 >= 0.0f && q.depth1 <= 255.0f, "depth0 or depth1 outside [0, 255]");
    REQUIRE(ctx, q.feather >= 0.0f, "feather must be >= 0");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kComposite, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    Effect::Composite &k = e.composite;
    k.layer = q; k.sprite = sprite; k.spritePitch = spritePitch;
    k.depthOut = depthOut; k.depthOutPitch = depthOut ? depthOutPitch : 0;
    // the footprint, clipped to the image; a sprite wholly outside leaves it empty (all 0) and the launch copies
    const int fx0 = std::max(q.x, 0), fx1 = std::min(q.x + layer_extent(q.cols, q.scale), cols);
    const int fy0 = std::max(q.y, 0), fy1 = std::min(q.y + layer_extent(q.rows, q.scale), rows);
    if (fx0 < fx1 && fy0 < fy1) { k.fx0 = fx0; k.fy0 = fy0; k.fx1 = fx1; k.fy1 = fy1; }
    return simulate(ctx, e);
}

int rtdd_remove_object(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const float *depth, size_t depthPitch,
                       const uint8_t *mask, size_t maskPitch, uint8_t *artistic, size_t artisticPitch, float *depthOut,
                       size_t depthOutPitch, int rows, int cols, const rtdd_removal *removal) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_effect(ctx, original, depth, artistic, originalPitch, depthPitch, artisticPitch, rows, cols);
    if (rc != RTDD_OK) return rc;
    if (depthOut) {
        REQUIRE(ctx, depthOutPitch >= (size_t)cols * 4, "pitch smaller than a row");
        REQUIRE(ctx, f32_image_aligned(depthOut, depthOutPitch), kF32AlignText);
    }
    REQUIRE(ctx, original != artistic && (const float *)depthOut != depth, "an object cannot be removed in place");
    REQUIRE(ctx, mask && maskPitch >= (size_t)cols, "bad mask image");
    REQUIRE(ctx, removal, "null removal");
    const rtdd_removal &q = *removal;
    REQUIRE(ctx, q.select >= 0 && q.select <= 255, "select outside [0, 255]");
    REQUIRE(ctx, q.grow >= 0 && q.grow <= 8, "grow outside [0, 8]");
    REQUIRE(ctx, std::isfinite(q.sourceMinDepth), "a non-finite value in the removal");
    REQUIRE(ctx, q.sourceMinDepth >= 0.0f && q.sourceMinDepth <= 255.0f, "sourceMinDepth outside [0, 255]");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kRemove, original, originalPitch, depth, depthPitch, artistic, artisticPitch, rows, cols};
    Effect::Remove &k = e.remove;
    k.removal = q; k.mask = mask; k.maskPitch = maskPitch;
    k.depthOut = depthOut; k.depthOutPitch = depthOut ? depthOutPitch : 0;
    return simulate(ctx, e);
}

int rtdd_lift_layer(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const uint8_t *mask, size_t maskPitch, int rows, int cols,
                    int select, int x, int y, uint8_t *sprite, size_t spritePitch, int spriteRows, int spriteCols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, original && mask && sprite, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    REQUIRE(ctx, (long long)rows * rows + (long long)cols * cols < 2147483647LL, "image too large");
    REQUIRE(ctx, originalPitch >= (size_t)cols * 3 && maskPitch >= (size_t)cols, "pitch smaller than a row");
    REQUIRE(ctx, original != sprite, "a sprite cannot be lifted in place");
    REQUIRE(ctx, spriteRows >= 1 && spriteRows <= 16384 && spriteCols >= 1 && spriteCols <= 16384, "the sprite's rows or cols outside [1, 16384]");
    REQUIRE(ctx, spritePitch >= (size_t)spriteCols * 4, "pitch smaller than a row");
    REQUIRE(ctx, select >= 0 && select <= 255, "select outside [0, 255]");
    REQUIRE(ctx, x >= -16384 && x <= 16383 && y >= -16384 && y <= 16383, "a sprite coordinate outside [-16384, 16383]");
    Effect e{Effect::kLift, original, originalPitch, nullptr, 0, nullptr, 0, rows, cols};      // (an empty image: a transparent sprite)
    Effect::Lift &k = e.lift;
    k.mask = mask; k.maskPitch = maskPitch; k.select = select; k.x = x; k.y = y;
    k.sprite = sprite; k.spritePitch = spritePitch; k.spriteRows = spriteRows; k.spriteCols = spriteCols;
    return simulate(ctx, e);
}

// rtdd_lift_layer's image rules for a mask-sized u8 image and its size (rtdd_mask_distance, rtdd_refine_mask)
static int check_mask(rtdd_ctx *ctx, const void *mask, size_t maskPitch, const void *out, int rows, int cols) {
    REQUIRE(ctx, mask && out, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    REQUIRE(ctx, (long long)rows * rows + (long long)cols * cols < 2147483647LL, "image too large");
    REQUIRE(ctx, maskPitch >= (size_t)cols, "pitch smaller than a row");
    REQUIRE(ctx, mask != out, "a mask cannot be refined in place");
    return RTDD_OK;
}

int rtdd_mask_distance(rtdd_ctx *ctx, const uint8_t *mask, size_t maskPitch, int rows, int cols, int select, int reach, int32_t *dist2,
                       size_t dist2Pitch) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_mask(ctx, mask, maskPitch, dist2, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, dist2Pitch >= (size_t)cols * 4, "pitch smaller than a row");
    REQUIRE(ctx, f32_image_aligned(dist2, dist2Pitch), kF32AlignText);
    REQUIRE(ctx, select >= 0 && select <= 255, "select outside [0, 255]");
    REQUIRE(ctx, reach >= 1 && reach <= kEdtMaxReach, "reach outside [1, 1024]");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kMaskDistance, nullptr, 0, nullptr, 0, nullptr, 0, rows, cols};
    Effect::MaskOp &k = e.maskop;
    k.mask = mask; k.maskPitch = maskPitch; k.select = select; k.reach = reach; k.dist2 = dist2; k.dist2Pitch = dist2Pitch;
    return simulate(ctx, e);
}

int rtdd_refine_mask(rtdd_ctx *ctx, const uint8_t *mask, size_t maskPitch, int rows, int cols, const rtdd_mask_refine *refine, uint8_t *out,
                     size_t outPitch) {
    if (!ctx) return RTDD_ERR_INVALID;
    int rc = check_mask(ctx, mask, maskPitch, out, rows, cols);
    if (rc != RTDD_OK) return rc;
    REQUIRE(ctx, outPitch >= (size_t)cols, "pitch smaller than a row");
    REQUIRE(ctx, refine, "null refine");
    const rtdd_mask_refine &q = *refine;
    REQUIRE(ctx, q.select >= 0 && q.select <= 255, "select outside [0, 255]");
    constexpr int kMax2 = kEdtMaxReach * kEdtMaxReach;
    // the reach: the smallest R with R^2 >= the largest threshold, or with R >= max(|lo|, |hi|) + 0.5 (include/rtdd.h: a pixel beyond it
    // saturates to the byte its true E gives it)
    int reach = 1;
    if (q.op == RTDD_REFINE_FEATHER) {
        REQUIRE(ctx, std::isfinite(q.lo) && std::isfinite(q.hi), "a non-finite value in the refine");
        REQUIRE(ctx, q.lo >= -1023.5f && q.hi <= 1023.5f && q.lo < q.hi, "the feather needs -1023.5 <= lo < hi <= 1023.5");
        reach = (int)std::ceil(std::max(std::fabs((double)q.lo), std::fabs((double)q.hi)) + 0.5);
    } else {
        int most = 0;
        if (q.op == RTDD_REFINE_GROW) { REQUIRE(ctx, q.outer2 >= 1 && q.outer2 <= kMax2, "outer2 outside [1, 1024^2]"); most = q.outer2; }
        else if (q.op == RTDD_REFINE_SHRINK) { REQUIRE(ctx, q.inner2 >= 1 && q.inner2 <= kMax2, "inner2 outside [1, 1024^2]"); most = q.inner2; }
        else if (q.op == RTDD_REFINE_OUTLINE) {
            REQUIRE(ctx, q.inner2 >= 0 && q.inner2 <= kMax2 && q.outer2 >= 0 && q.outer2 <= kMax2, "inner2 or outer2 outside [0, 1024^2]");
            REQUIRE(ctx, q.inner2 != 0 || q.outer2 != 0, "an outline needs inner2 or outer2");
            most = std::max(q.inner2, q.outer2);
        } else return fail(ctx, RTDD_ERR_INVALID, "op must be RTDD_REFINE_GROW, _SHRINK, _OUTLINE or _FEATHER");
        while (reach * reach < most) reach++;
    }
    REQUIRE(ctx, reach >= 1 && reach <= kEdtMaxReach, "the refine reaches beyond 1024 pixels");
    if (rows == 0 || cols == 0) return RTDD_OK;
    Effect e{Effect::kRefineMask, nullptr, 0, nullptr, 0, nullptr, 0, rows, cols};
    Effect::MaskOp &k = e.maskop;
    k.mask = mask; k.maskPitch = maskPitch; k.select = q.select; k.reach = reach; k.refine = q; k.out = out; k.outPitch = outPitch;
    return simulate(ctx, e);
}

int rtdd_lift_layer_matte(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch, const uint8_t *alpha, size_t alphaPitch, int rows, int cols,
                          int x, int y, uint8_t *sprite, size_t spritePitch, int spriteRows, int spriteCols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, original && alpha && sprite, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0, "negative size");
    REQUIRE(ctx, (long long)rows * rows + (long long)cols * cols < 2147483647LL, "image too large");
    REQUIRE(ctx, originalPitch >= (size_t)cols * 3 && alphaPitch >= (size_t)cols, "pitch smaller than a row");
    REQUIRE(ctx, original != sprite, "a sprite cannot be lifted in place");
    REQUIRE(ctx, spriteRows >= 1 && spriteRows <= 16384 && spriteCols >= 1 && spriteCols <= 16384, "the sprite's rows or cols outside [1, 16384]");
    REQUIRE(ctx, spritePitch >= (size_t)spriteCols * 4, "pitch smaller than a row");
    REQUIRE(ctx, x >= -16384 && x <= 16383 && y >= -16384 && y <= 16383, "a sprite coordinate outside [-16384, 16383]");
    Effect e{Effect::kLiftMatte, original, originalPitch, nullptr, 0, nullptr, 0, rows, cols};  // (an empty image: a transparent sprite)
    Effect::Lift &k = e.lift;
    k.mask = alpha; k.maskPitch = alphaPitch; k.select = 0; k.x = x; k.y = y;
    k.sprite = sprite; k.spritePitch = spritePitch; k.spriteRows = spriteRows; k.spriteCols = spriteCols;
    return simulate(ctx, e);
}

}  // extern "C"
#pragma GCC visibility pop
