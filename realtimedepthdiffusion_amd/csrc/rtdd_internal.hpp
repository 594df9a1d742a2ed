// rtdd_internal.hpp -- private declarations shared by the translation units of librtdd.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rtdd.h"

namespace rtdd {

// ---- internal plane geometry ------------------------------------------------------------------
// Solver state lives in dense private planes (x_k, x_{k-1}/x_{k+1}, packed per-pixel metadata),
// NOT in the caller's pitched buffers.  A plane has `ip` elements per row with at least
// kGuardCols unused elements after the last image column (they double as the left guard of the
// next row) and kGuardRows unused rows before row 0 and after the last row, so stencil/halo
// loads never need bounds checks on the ADDRESS -- only on whether the value is used.
constexpr int kGuardRows = 16;
constexpr int kGuardCols = 64;
constexpr int kRowAlign = 64;       // ip is a multiple of 64 elements = 256 B

inline size_t plane_pitch(int cols) { return (size_t)((cols + kRowAlign - 1) / kRowAlign) * kRowAlign + kGuardCols; }
inline size_t plane_elems(int rows, int cols) { return plane_pitch(cols) * (size_t)(rows + 2 * kGuardRows) + 1024; }

// packed per-pixel metadata: bits 0-7 edge-weight index to the RIGHT neighbour, 8-15 index to the
// neighbour BELOW, bit 16 = Dirichlet (scribble == 255).  Left/up indices are the right/down
// indices of the left/upper neighbour (|a-b| and the depth gate are symmetric,
// /root/reference/src/GPUSolver.cu:188-218); "no neighbour" (256) follows from coordinates.
constexpr uint32_t kMetaDirichlet = 1u << 16;

struct Level {
    int rows = 0, cols = 0;         // allocation size (upper bound for solve calls)
    size_t elems = 0;               // elements per plane
    float *plane[4] = {nullptr, nullptr, nullptr, nullptr};   // raw allocations (4 f32 planes)
    uint32_t *meta = nullptr;
    // views at row 0 (after the guard rows)
    float *P(int i, size_t ip) const { return plane[i] + (size_t)kGuardRows * ip; }
    uint32_t *M(size_t ip) const { return meta + (size_t)kGuardRows * ip; }
    // A context created for a batch of images (rtdd_pyramid_create_batch) allocates every plane `images` times over, image b's copy
    // `elems` elements behind image b - 1's: view(b) is the level as image b sees it.
    Level view(int b) const {
        Level v = *this;
        for (auto &q : v.plane) if (q) q += (size_t)b * elems;
        if (v.meta) v.meta += (size_t)b * elems;
        return v;
    }
};

// The images a batched launch covers (rtdd_estimate_depth_batch; BASELINE configs[3]: independent images on one GPU): blockIdx.z = image
// index - first.  Every kernel on the estimate's path takes, next to each image pointer, the BYTE stride between consecutive images of
// that argument (0 and gridDim.z = 1 for everything else).  Planes of the solver: Level::elems * 4.
struct Batch {
    int n = 1;                            // images per launch
    int first = 0;                        // the first one's index in the context's batched allocations
    size_t depth = 0, scribble = 0, gray = 0, u8 = 0;     // byte strides of the caller-side arguments of the solve in progress (gray: the guide's, gray or colour)
    size_t regions = 0;                   // ... and of its region codes (SolveCall::regions)
};
#define RTDD_Z(ptr, stride) ptr = (decltype(ptr))((const char *)(ptr) + (size_t)blockIdx.z * (size_t)(stride))

// What a solve is told BESIDES the reference's own arguments (GPUMatrixFreeSolver's, src/GPUSolver.cu:274-275): part of its SolveCall.
struct SolveTargets {
    Batch batch;                                    // the images the launches cover (n = 1, first = 0: one image)
    bool defer_finish = false;                      // leave the result in its plane: the next level's pyrUp kernel reads it there
    uint8_t *u8 = nullptr; size_t u8_pitch = 0;     // the copy-back kernel also writes the u8 map here (src/main.cpp:290) ...
    uint8_t *u8b = nullptr; size_t u8b_pitch = 0;   // ... and a second copy here (a live frame's staging slot or the host's buffer)
    bool logged = true;                             // false: a step of a larger logged call (an estimate's per-level solves)
};
// What a solve hands back to a caller inside the library: its sequence number (what the guarded copy-back kernels report) and the
// plane its result is in (defer_finish).
struct SolveOutcome { int seq = 0, plane = -1; };
// One solve: what rtdd_solve_ex is given plus what the library's own callers add.  Built once per entry point (rtdd_solve_ex,
// rtdd_matrix_free_solver, estimate_levels, rtdd_refine_depth), passed down by const reference -- solve_with -> solve_once -> the
// launchers -- and stored by value in the pending-call log (PendingOp): nothing is parked in the context around a call, so a replay
// hands the stored record straight back.  The sequence number and the SolveOutcome are per attempt, not per call, and travel beside it.
struct SolveCall {
    float *depth = nullptr; size_t depthPitch = 0;
    const uint8_t *scribble = nullptr; size_t scribblePitch = 0;
    const uint8_t *gray = nullptr; size_t grayPitch = 0;
    int guide = RTDD_GUIDE_GRAY;                    // rtdd_guide: what `gray` points at -- a gray image, or (RTDD_GUIDE_BGR) the interleaved colour image
    int rows = 0, cols = 0, level = 0;
    rtdd_solve_params params{};
    SolveTargets targets;                           // (rtdd_refine_depth: the selected image of a batch, the u8 copy of the result)
    // depth regions (rtdd_solve_regions): one u8 code per pixel and rtdd_region_flags.  regionFlags == 0: no regions -- `regions` is
    // null, nothing of them is launched, the call is rtdd_solve_guided.  Part of the record, so a replay runs a region solve with regions
    const uint8_t *regions = nullptr; size_t regionsPitch = 0;
    int regionFlags = 0;
};
// A live frame's own images (live.cpp): the level-0 annotation pair its estimate ran on, the second target of its u8 map
// (u8_pitch 0: a staging slot with the pyramid's pitch), and the sticky depth effect behind it (src/main.cpp:190-230) with its target.
struct LiveTargets {
    void *scribble = nullptr, *edited = nullptr;
    uint8_t *u8 = nullptr; size_t u8_pitch = 0;
    int effect = 0;                                 // RTDD_EFFECT_*
    uint8_t *artistic = nullptr; size_t artistic_pitch = 0;     // device image the effect writes (the frame's staging slot)
};

// One depth effect, arguments checked: what to render, on which images, with which parameters.  Built by the rtdd_simulate_* entry
// points (effects_api.cpp) and by a live frame (live_effect), launched by launch_effect, and logged by value (PendingOp) to be launched again.
struct Effect {
    enum : int { kRefocus = RTDD_EFFECT_HAZE + 1, kHazeEx, kStereo, kLensBlur, kRelight, kRelightShadow, kParallax, kAmbientOcclusion, kLighting, kBokeh, kComposite, kRemove, kLift, kParallaxLayered, kMaskDistance, kRefineMask, kLiftMatte };   // the extensions, after the public kinds
    int kind = RTDD_EFFECT_NONE;                    // RTDD_EFFECT_DEFOCUS / _DESATURATION / _HAZE, kRefocus, kHazeEx, kStereo, kLensBlur, kRelight, kRelightShadow, kParallax, kAmbientOcclusion, kLighting, kBokeh, kComposite, kRemove, kLift, kParallaxLayered, kMaskDistance, kRefineMask, kLiftMatte
    const uint8_t *original = nullptr; size_t originalPitch = 0;
    const float *depth = nullptr; size_t depthPitch = 0;
    uint8_t *artistic = nullptr; size_t artisticPitch = 0;
    int rows = 0, cols = 0;
    const uint8_t *gray = nullptr; size_t grayPitch = 0;            // desaturation
    // refocus, lens blur (the round aperture; the square one IS a refocus), bokeh (<= 127): the window scale (<= 255) and the focus (focusX >= 0: the map's pixel (focusX, focusY), read by the kernels when they run)
    int kernelSize = 0, focusX = -1, focusY = -1;
    float focusDepth = 0.0f;
    float beta = 2.0f; uint32_t air = 0xFFFFFFu;                    // haze_ex: density and airlight b | g << 8 | r << 16
    // stereo: disparity (|D| <= 256), zero parallax (zeroX >= 0: the map's pixel (zeroX, zeroY), read by the kernel), rtdd_stereo_mode
    int disparity = 0, zeroX = -1, zeroY = -1, stereoMode = 0;
    float zeroDepth = 0.0f;
    // relight: the light as the host prepared it (include/rtdd.h rtdd_simulate_relight), by value -- a replay needs no rtdd_light
    struct Light {
        int kind = 0, anchorX = -1, anchorY = -1;   // rtdd_light_kind; anchorX >= 0: the map's pixel (anchorX, anchorY), read by the kernel
        float x = 0.0f, y = 0.0f, z = 1.0f;         // directional: the unit vector towards the light; point: position (pixels) and height above the anchor
        float anchorDepth = 0.0f, invR2 = 0.0f;     // point
        float relief = 0.0f, ambient = 0.0f, k[3] = {0.0f, 0.0f, 0.0f};   // k[c] = diffuse * colour_c / 255 for c of B, G, R
    } light = {};
    // relight with cast shadows (kRelightShadow: `light` too): the march as the host prepared it (include/rtdd.h
    // rtdd_simulate_relight_shadowed), by value.  sx, sy, rise: a directional light's step along the major axis (sx == sy == 0: the
    // light stands straight above, m == 0, every pixel is lit); a point light's are per pixel, the kernel's.
    struct Shadow {
        float sx = 0.0f, sy = 0.0f, rise = 0.0f;
        int maxSteps = 0;
        float bias = 0.0f, softness = 0.0f, strength = 0.0f;
    } shadow = {};
    // parallax (kParallax): the view as rtdd_parallax states it (include/rtdd.h rtdd_simulate_parallax) and the image centre the host
    // computed, by value -- a replay needs no rtdd_parallax.  zeroX >= 0: the map's pixel (zeroX, zeroY), read by the kernel
    struct Parallax {
        int shiftX = 0, shiftY = 0, zeroX = -1, zeroY = -1;
        float dolly = 0.0f, zeroDepth = 0.0f;
        float cx = 0.0f, cy = 0.0f;                 // (float)(cols - 1) * 0.5f, (float)(rows - 1) * 0.5f
    } parallax = {};
    // the two-layer parallax view (kParallaxLayered, include/rtdd.h rtdd_simulate_parallax_layered): `parallax` as above, and the back
    // layer and the two extra outputs, by value; each null when the call had none.  All of them null: rtdd_simulate_parallax's launches
    struct ParallaxLayers {
        const uint8_t *plate = nullptr; size_t platePitch = 0;
        const float *plateDepth = nullptr; size_t plateDepthPitch = 0;
        float *depthOut = nullptr; size_t depthOutPitch = 0;
        uint8_t *coverage = nullptr; size_t coveragePitch = 0;
    } layers = {};
    // ambient occlusion (kAmbientOcclusion): rtdd_ambient_occlusion as the entry point checked it (include/rtdd.h
    // rtdd_simulate_ambient_occlusion), by value -- a replay needs no rtdd_ambient_occlusion.  lit: the call had a light, prepared in
    // `light` as relight's (light.relief == relief bit for bit); the tables inv_j[k] depend on k alone and are the launcher's.
    // The whole lighting model (kLighting, include/rtdd.h rtdd_simulate_lighting) has no fields of its own: `light`, `shadow` and
    // `occlusion` (lit, RTDD_AO_SHADE) as the three calls prepare them
    struct Occlusion {
        int mode = 0, directions = 8, radius = 0;   // rtdd_ao_mode; 4 or 8; [0, 64]
        float relief = 0.0f, bias = 0.0f, strength = 0.0f;
        bool lit = false;
    } occlusion = {};
    // a composited layer (kComposite): rtdd_layer as the entry point checked it (include/rtdd.h rtdd_composite_layer), the sprite and the
    // second output, by value -- a replay needs no rtdd_layer.  The footprint: the image pixels [fx0, fx1) x [fy0, fy1) the sprite covers,
    // clipped to the image (all 0: none, the launch copies); a pixel outside it is uncovered, one inside it is tested by the kernel
    struct Composite {
        rtdd_layer layer = {};
        const uint8_t *sprite = nullptr; size_t spritePitch = 0;
        float *depthOut = nullptr; size_t depthOutPitch = 0;       // null: no depth is written
        int fx0 = 0, fy0 = 0, fx1 = 0, fy1 = 0;
    } composite = {};
    // a removed object (kRemove): rtdd_removal as the entry point checked it (include/rtdd.h rtdd_remove_object), the mask and the second
    // output, by value
    struct Remove {
        rtdd_removal removal = {};
        const uint8_t *mask = nullptr; size_t maskPitch = 0;
        float *depthOut = nullptr; size_t depthOutPitch = 0;       // null: no depth is written
    } remove = {};
    // a lifted sprite (kLift, rtdd_lift_layer): reads original (rows x cols) and the mask, writes the sprite; depth and artistic are null
    // (kLiftMatte, rtdd_lift_layer_matte: `mask` is the alpha image, select 0)
    struct Lift {
        const uint8_t *mask = nullptr; size_t maskPitch = 0;
        int select = 0, x = 0, y = 0;
        uint8_t *sprite = nullptr; size_t spritePitch = 0;
        int spriteRows = 0, spriteCols = 0;
    } lift = {};
    // a mask's distance transform (kMaskDistance, rtdd_mask_distance: writes dist2) or a refined mask (kRefineMask, rtdd_refine_mask:
    // `refine` as the entry point checked it, by value, `reach` derived from it; writes out); original, depth and artistic are null
    struct MaskOp {
        const uint8_t *mask = nullptr; size_t maskPitch = 0;
        int select = 0, reach = 0;
        int32_t *dist2 = nullptr; size_t dist2Pitch = 0;
        rtdd_mask_refine refine = {};
        uint8_t *out = nullptr; size_t outPitch = 0;
    } maskop = {};
};

// The defocus window scale K of src/GPUDepthEffect.cu:42, (int)(aperture * diagonal) -- double * float and the int products as there,
// evaluated on the host (sqrtf is correctly rounded on the host as on the device).  INT_MAX where the product does not fit an int (an
// aperture a refocus refuses).
inline int window_scale(double aperture, int rows, int cols) {
    const double k = aperture * sqrtf(rows * rows + cols * cols);
    return k < 2147483647.0 ? (int)k : 2147483647;
}

struct Options {
    int fp_contract = 1;
    int sweep_kernel = 0;
    int temporal_depth = 0;
    int rows_per_wave = 0;
    int tile = 0;
    int persistent = 1;
    int defocus_path = 0;                // RTDD_OPT_DEFOCUS_PATH: 0 automatic, 1 global summed-area table, 2 per-tile tables in LDS where they fit
    // RTDD_METHOD_AUTO's cost model (constants, not clocks: a solve is reproducible).  Readable and settable as options so that
    // what decided a solve can be restated from outside (tests/test_gpu_multigrid.py).
    int auto_cycle_fixed_ns = 270000;    // a V-cycle with its residual check: launch-bound part ...
    int auto_cycle_fs_per_px = 46000;    // ... plus streaming part per level-0 pixel (femtoseconds)
    int auto_sweep_fs_per_px = 1429;     // one red-black sweep per pixel (1 / 700 Gpx-sweeps/s) ...
    int auto_sweep_floor_ns = 2500;      // ... but never below one launch-bound sweep
    int debug_withhold_tile = 0;     // RTDD_OPT_DEBUG_WITHHOLD_TILE: tile number + 1 whose exchange flag is never published (0 = off)
    int debug_poll_limit_us = 0;     // RTDD_OPT_DEBUG_POLL_LIMIT_US: exchange poll limit (0 = default, 200 ms)
    int debug_force_status = 0;      // RTDD_OPT_DEBUG_FORCE_STATUS: one-shot value for the status word behind the next blocked launch
    int timeout_heal = 1;            // RTDD_OPT_TIMEOUT_HEAL: 1 a timed-out persistent launch is healed (calls logged, run again); 0 it is reported
    int annotation_lds = 1;          // RTDD_OPT_ANNOTATION_LDS: the annotation pyramid's chain of levels in LDS (pyramids of up to 6 levels); 0: through global memory
    int live_zero_copy = 1;          // RTDD_OPT_LIVE_ZERO_COPY: a live frame's u8 map is stored by the copy-back kernel straight into the host's page-locked buffer (0 never, 1 when no other frame is in flight, 2 always)
    int defocus_slice_mb = 0;        // RTDD_OPT_DEFOCUS_SLICE_MB: > 0: a summed-area table of more than twice this is built and looked up in slices of at most this size
    int defocus_strips = 0;          // RTDD_OPT_DEFOCUS_STRIPS: the table lookup's tile order -- 0 automatic, 1 row bands per XCD, 2 column strips per XCD
    int rearm_after = 64;            // RTDD_OPT_PERSISTENT_REARM_AFTER: solves without persistence after the first heal, doubling with every further one
};

// One asynchronous call whose results the caller has not yet seen confirmed by a synchronising call: what check_persistent_status
// needs to run it again when a persistent launch gave up (heal.cpp).  One record per kind, side by side (the log holds at most
// kMaxPendingOps entries): `kind` says which one is meant, and replay hands it back to solve_with / estimate_replay / launch_effect as
// it is.  A solve is one sequence number (handed to the kernel that publishes its result: k_finish, or k_pyrup_inject inside an
// estimate); an estimate is one per pyramid level; an effect publishes none.
struct PendingOp {
    enum Kind { kSolve = 0, kEstimate = 1, kEffect = 2 } kind = kSolve;
    Options opt;                          // the options in force when the call was made
    unsigned long long id = 0;            // position in the context's call order (live mode drops the confirmed prefix of the log)
    SolveCall solve;                      // kSolve ...
    int seq = 0;                          // ... and its sequence number
    struct Estimate {                     // kEstimate
        int maxIterations = 0;
        int level_seq[32] = {};           // sequence number of level l's solve (0: the level is empty)
        int batch_first = 0, batch_n = 1; // the images of the context's batched pyramid the estimate covers
        int guide = RTDD_GUIDE_GRAY;      // the guide the estimate ran with (rtdd_pyramid_set_guide): a replay uses it, not the pyramid's current one
        int regionFlags = 0;              // ... and the rtdd_region_flags (rtdd_pyramid_set_regions): likewise; the code planes are read as they are
        LiveTargets live;                 // a live frame: its annotation pair, its map's second target, its effect (scribble == nullptr: not one)
        // what the estimate did to the coarse annotation levels in front of its solves: kAnnotationNone (they were up to date),
        // kAnnotationAccumulated (GPUPyrDownAnnotation: only ever adds) or kAnnotationRebuilt (as if they had been all zero).  A replay
        // of a rebuilt estimate rebuilds them again from the annotation pair it ran on, and the accumulating estimates replayed behind
        // it add theirs again: a newer live frame's strokes, accumulated in the meantime, are gone from the older frame's Dirichlet set
        int annotation = 0;
    } estimate;
    enum : int { kAnnotationNone = 0, kAnnotationAccumulated = 1, kAnnotationRebuilt = 2 };
    Effect effect;                        // kEffect: queued BEHIND an unconfirmed solve (it may have read that solve's input, not its result)
};
constexpr int kRestartSolve = -1000;      // internal status: the pending calls were healed inside a solve's residual check; that solve starts over
constexpr size_t kMaxPendingOps = 4096;
constexpr int kMaxRearms = 4;             // heals after which persistence stays off for the context's life

}  // namespace rtdd

namespace rtdd { struct Pyramid; struct MgState; }

namespace rtdd {
// A contiguous device buffer a host image with an unaligned pitch goes through (one per stream that copies: uses of one buffer are
// ordered by that stream).
struct Bounce { void *ptr = nullptr; size_t bytes = 0; };
}

struct rtdd_ctx {
    int device = 0;
    rtdd::Pyramid *pyr = nullptr;       // whole-estimate driver state (pyramid.hpp)
    rtdd::MgState *mg = nullptr;        // multigrid hierarchy buffers (multigrid.hip), kept between solves of one size
    hipStream_t stream = nullptr;
    std::vector<rtdd::Level> levels;
    int alloc_images = 1;               // how many images' planes the NEXT rtdd_allocate makes every level hold (rtdd_pyramid_create_batch; one shot)
    int levels_images = 1;              // ... and how many the levels hold now
    int maxLevel = -1;
    bool weights_loaded = false;
    float lut_host[257];
    float *lut_dev = nullptr;
    float *omega_dev = nullptr;     // device copy of the omega schedule (temporally blocked kernel)
    int omega_cap = 0;
    float *residual_dev = nullptr;  // extension: residual reduction target
    int *sync_words = nullptr;      // control words of the persistent kernels (persist_sync.hpp); allocated with the context
    int defocus_last_path = 0;           // RTDD_OPT_DEFOCUS_LAST_PATH: what the most recent rtdd_simulate_defocus launched (1 table, 2 tile kernel)
    int defocus_last_slices = 0;         // ... and, on the table path, how many horizontal slices it built a table for (1: one whole-image table)
    bool defocus_band_sticky = false;    // a banded-table defocus met windows beyond a slice (depths above 255): one whole-image table from then on
    bool defocus_table_sticky = false;   // a tile-kernel defocus met out-of-range depths (seen at a synchronisation): automatic choice = the table from then on
    int flag_epoch = 0;             // the per-tile flags of the persistent kernels only ever grow: base value of the next persistent launch (heal.cpp)
    int sync_limit = 0;             // what sync_words[kSyncLimit] currently holds on the device
    int last_nominal_depth = 0;     // sweeps per launch / exchange the most recent blocked solve was configured with (its last launch may be shorter)
    int last_launch_images = 1;     // images each sweep launch of the most recent solve covered (sweep_blocked.hip: a batch in the same launches, or image after image)
    rtdd_solve_info last_info{};    // of the most recent solve; kernel/tile/temporal_depth/persistent are filled in by the sweep launchers
    // Self-healing after RTDD_ERR_TIMEOUT (heal.cpp): every solve / estimate since the last status check, in call order
    int solve_seq = 0;              // sequence number of the most recent rtdd_solve_ex (1 .. 2^30, never 0)
    int wild_seq = -1;              // the number the solve being queued hands k_prepare and its sweep kernels (persist_sync.hpp kSyncWild);
                                    // -1 outside a solve (the diagnostics of scripts/ubench launch sweeps directly): never the word's value
    std::vector<rtdd::PendingOp> pending;
    bool pending_overflow = false;  // more than kMaxPendingOps calls without a synchronisation: a timeout among them is reported, not healed
    bool healing = false;           // a replay is running: nothing is logged, a second timeout is final
    bool heal_rebuilt = false;      // ... and one of the estimates run again so far has rebuilt the coarse annotation levels (PendingOp::annotation)
    bool heal_warned = false;
    int heals = 0;                  // RTDD_OPT_TIMEOUT_HEALS
    // opt.persistent is what the launchers read; persistent_wanted is what the caller asked for.  A heal switches opt.persistent off and
    // suspends it for persist_suspend more solves (rearm_after, doubling with every heal; -1 after kMaxRearms heals: off for good)
    int persistent_wanted = 1;
    int persist_suspend = 0;        // RTDD_OPT_PERSISTENT_SUSPENDED
    int *confirm_host = nullptr;    // page-locked: sequence number of the latest solve whose copy-back kernel published its result (persist_sync.hpp)
    unsigned long long op_counter = 0;
    bool persistent_used = false;   // a launch that can set the status word (sync_words[kSyncStatus]) happened since the last status check
    // The copy-back kernels report in page-locked memory the sequence number of a solve they published WITH THE STATUS WORD CLEAR
    // (confirm_host).  If the newest such kernel launched (publish_seq) has reported, and nothing that can set a control word has been
    // launched behind it (status_writer_behind), a synchronised stream proves the words clear without reading them from the device: the
    // drop-in shim synchronises behind every pyramid level's solve, and the 32-byte blocking hipMemcpy was most of what that cost it.
    int publish_seq = 0;
    bool status_writer_behind = false;
    signed char persist_fit[17][2];  // per (tile id, contraction): does one workgroup of the persistent kernel fit a CU of THIS device (-1 = not asked yet)
    rtdd::Bounce bounce;            // host <-> device 2-D copies with an unaligned host pitch, on ctx->stream (copy_h2d / copy_d2h, image_api.cpp)
    uint32_t *sat = nullptr;        // defocus summed-area table scratch; the parallax view's keys
    size_t sat_elems = 0;
    int sat_rows = 0, sat_cols = 0;     // the geometry the table's zero padding was laid out for (effect_kernels.hip)
    int num_cus = 256;
    rtdd::Options opt;
    bool profile_on = false;
    rtdd_profile prof{};
    // profiling: 4 events per solve call, a ring of kProfSlots calls; resolved lazily by rtdd_profile_get (no sync per call)
    static constexpr int kProfSlots = 64;
    hipEvent_t ev[4 * kProfSlots] = {};
    int prof_launches[kProfSlots] = {}, prof_sweeps[kProfSlots] = {};
    int prof_pending = 0;           // calls recorded since the last rtdd_profile_get
    std::string last_error;
};

namespace rtdd {

#ifdef __HIPCC__
// A thread's wave number within its workgroup as a SCALAR (every lane of a wave holds the same value; v_readfirstlane tells the compiler
// so): row indices and row pointers derived from it are then computed once per wave on the scalar unit.  Left as `threadIdx.x >> 6` they
// are per-lane values, and `(size_t)y * pitch` becomes two v_mul_lo_u32 and a v_mad_u64_u32 per row pointer -- quarter-rate
// instructions: 17 of them in the desaturation kernel, 16 in k_prepare4, 31 in k_pyrup_inject4 (round 4: all but one gone; the streaming
// kernels are memory-bound, so it bought them only 1-9 %: EXPERIMENTS.md).
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
#endif

int fail(rtdd_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess);
// The f32 alignment contract of include/rtdd.h: every entry point that takes an f32 image refuses one whose pointer or pitch is no
// multiple of 4 (the kernels read and write it as floats; u8 images are legal at any pointer and pitch).
inline bool f32_image_aligned(const void *p, size_t pitch) { return (uintptr_t)p % sizeof(float) == 0 && pitch % sizeof(float) == 0; }
constexpr const char *kF32AlignText = "an f32 image needs a pointer and a pitch that are multiples of 4";
// a launch that can set one of the control words (sync_words) has been queued: the next synchronising call must look at them
inline void note_status_writer(rtdd_ctx *ctx) { ctx->persistent_used = true; ctx->status_writer_behind = true; }
// a guarded copy-back kernel (k_finish, k_pyrup_inject) for solve `seq` has been queued: it reports `seq` if it finds the words clear
inline void note_publisher(rtdd_ctx *ctx, int seq) { ctx->persistent_used = true; ctx->publish_seq = seq; ctx->status_writer_behind = false; }

#define RTDD_HIP(ctx, call)                                                        \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) return ::rtdd::fail((ctx), RTDD_ERR_HIP, #call, e_); \
    } while (0)

#define REQUIRE(ctx, cond, msg) \
    do { if (!(cond)) return ::rtdd::fail((ctx), RTDD_ERR_INVALID, msg); } while (0)
// the first line of every entry point that works on the context's pyramid
#define REQUIRE_PYRAMID(ctx)                                                                                             \
    do {                                                                                                                 \
        if (!(ctx)) return RTDD_ERR_INVALID;                                                                             \
        if (!(ctx)->pyr) return ::rtdd::fail((ctx), RTDD_ERR_STATE, "rtdd_pyramid_create has not been called");          \
    } while (0)
// evaluate a call that returns an rtdd status; leave the function with it unless it is RTDD_OK
#define RTDD_TRY(call) \
    do { const int rc_ = (call); if (rc_ != RTDD_OK) return rc_; } while (0)

#define RTDD_LAUNCH_CHECK(ctx, name)                                                     \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) return ::rtdd::fail((ctx), RTDD_ERR_HIP, "launch " name, e_); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---- solver_kernels.hip -------------------------------------------------------------------------
// (c.targets.batch: the images a batched launch covers; L is its first image's view of the level)
int launch_prepare(rtdd_ctx *ctx, const Level &L, size_t ip, const SolveCall &c);
// Both sweep launchers advance n sweeps from (plane *pk = x_k, plane *pm = x_{k-1}) and update *pk / *pm to
// the planes holding x_{k+n} / x_{k+n-1}.
int launch_sweeps(rtdd_ctx *ctx, const Level &L, size_t ip, int rows, int cols, const float *omegas_host, int n,
                  int *pk, int *pm, int *launches);
// sweep_blocked.hip
int launch_sweeps_blocked(rtdd_ctx *ctx, const Level &L, size_t ip, int rows, int cols, const float *omegas_dev, int n,
                          int *pk, int *pm, int *launches, int images = 1);
// (k_finish and k_pyrup_inject store NOTHING when the status word is set: a timed-out solve leaves the caller's buffers as they were;
// the first of them to find it set records ctx->guard_seq in sync_words[kSyncFailedSeq])
// (seq: the solve's sequence number, reported by the kernel either as confirmed or as the first failed one; c.targets: the batch and the u8 targets)
int launch_finish(rtdd_ctx *ctx, const Level &L, size_t ip, int src_plane, const SolveCall &c, int seq);
// (regionFlags != 0: the rule of rtdd_solve_regions on top, from the code image `regions`)
int launch_index_to_weight(rtdd_ctx *ctx, const uint8_t *gray, size_t grayPitch, const float *depth, size_t depthPitch,
                           int32_t *index2, int level, int rows, int cols, int guide = RTDD_GUIDE_GRAY,
                           const uint8_t *regions = nullptr, size_t regionsPitch = 0, int regionFlags = 0);
int launch_residual(rtdd_ctx *ctx, const Level &L, size_t ip, int plane, int rows, int cols, float *host_out);
int launch_rbgs(rtdd_ctx *ctx, const Level &L, size_t ip, int plane, int rows, int cols, int nsweeps, float omega);
// ---- multigrid.hip ------------------------------------------------------------------------------
int launch_multigrid(rtdd_ctx *ctx, const Level &L0, size_t ip, int rows, int cols, int max_cycles, float tolerance, int check_every, double alternative_seconds,
                     double cycle_seconds, int *plane, int *cycles_done, float *residual, int *launches);
void mg_release(rtdd_ctx *ctx);
int mg_download(rtdd_ctx *ctx, int level, int which, float *host, int *rows, int *cols);

int launch_rbgs_blocked(rtdd_ctx *ctx, const Level &L, size_t ip, int rows, int cols, int n, float omega, int *plane, int *launches, int keep = -1);

// ---- image_kernels.hip --------------------------------------------------------------------------
// (images, z*: a batched launch over `images` images whose arguments lie z* bytes apart)
int launch_convert(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, float *dst, size_t dstPitch,
                   const uint8_t *mask, size_t maskPitch, int rows, int cols, int images = 1, size_t zSrc = 0, size_t zDst = 0, size_t zMask = 0);
int launch_pyrdown_annotation(rtdd_ctx *ctx, const uint8_t *ps, size_t psp, const uint8_t *pe, size_t pep, int prows, int pcols,
                              uint8_t *cs, size_t csp, uint8_t *ce, size_t cep, int crows, int ccols,
                              int images = 1, size_t zPs = 0, size_t zPe = 0, size_t zCs = 0, size_t zCe = 0);
// the annotation pyramid of an estimate (levels 1 .. levels-1 from level 0) and the coarsest level's injection, one launch (image_kernels.hip)
int launch_annotation_pyramid(rtdd_ctx *ctx, int levels, uint8_t *const *scribble, const size_t *sp, const size_t *zs, uint8_t *const *edited, const size_t *ep, const size_t *ze,
                              const int *rows, const int *cols, float *depth, size_t dp, size_t zd, int images, bool rebuild = false);
int launch_repitch(rtdd_ctx *ctx, hipStream_t stream, const void *src, size_t srcPitch, void *dst, size_t dstPitch, size_t widthBytes, int rows);
// ---- image_api.cpp: copies between host and device images ---------------------------------------
// hipMemcpy2DAsync between host and device takes ~9 us PER ROW when the host pitch is no multiple of four -- 8 ms for one plane of a
// 910-pixel-wide image (the dataset's Arara) where an aligned pitch takes 25 us (profiles/r05_copy2d_pitch.txt): slow_pitch.  A host
// image with such a pitch whose rows are contiguous (what a continuous cv::Mat or a numpy array is) moves as ONE linear copy through a
// contiguous device buffer and a re-pitching kernel (wants_bounce); any other layout takes the runtime's copy as it is.
inline bool slow_pitch(size_t hostPitch, int rows) { return hostPitch % 4 != 0 && rows > 1; }
inline bool wants_bounce(size_t hostPitch, size_t widthBytes, int rows) { return slow_pitch(hostPitch, rows) && hostPitch == widthBytes; }
// copy_h2d is its two halves on one stream.  The first leaves the host on copyStream: straight into the device image, or (wants_bounce)
// linearly into `b`, whose uses kernelStream orders; the second re-pitches `b` into the device image on kernelStream (nothing to do
// for a copy that went straight).  A live frame puts an event between them (live.cpp).
int copy_h2d_linear(rtdd_ctx *ctx, Bounce &b, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows,
                    hipStream_t copyStream, hipStream_t kernelStream);
int copy_h2d_repitch(rtdd_ctx *ctx, const Bounce &b, void *dev, size_t devPitch, size_t hostPitch, size_t widthBytes, int rows, hipStream_t kernelStream);
int copy_h2d(rtdd_ctx *ctx, Bounce &b, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows, hipStream_t stream);
int copy_d2h(rtdd_ctx *ctx, Bounce &b, void *host, size_t hostPitch, const void *dev, size_t devPitch, size_t widthBytes, int rows, hipStream_t stream);
// what the paint calls write: the annotation pair, the original an eraser restores from (null: none given), the size of all three
struct PaintTarget {
    uint8_t *edited; size_t editedPitch;
    uint8_t *scribble; size_t scribblePitch;
    const uint8_t *original; size_t originalPitch;
    int rows, cols;
};
int launch_paint(rtdd_ctx *ctx, int x, int y, int color, int radius, const PaintTarget &t);
// rtdd_paint_strokes / rtdd_paint_ramp_strokes (Stroke = rtdd_stroke / rtdd_ramp_stroke: the kernel's constant and ramp variants; a ramp's
// second label rides in the 12-byte record's spare bits): `count` checked strokes in array order, kStrokeChunk per launch (the records
// are kernel arguments)
template <class Stroke> int launch_paint_strokes(rtdd_ctx *ctx, const Stroke *strokes, int count, const PaintTarget &t);

// ---- fill_polygon.hip ---------------------------------------------------------------------------
// rtdd_fill_polygon: the checked contour (1 <= n <= 768 vertices, as kernel arguments) in one launch over its clipped bounding box
int launch_fill_polygon(rtdd_ctx *ctx, const int *xy, int n, const rtdd_fill &fill, const PaintTarget &t);

// ---- fill_similar.hip ---------------------------------------------------------------------------
// rtdd_fill_similar: the checked wand on three given images; grows the selection in rounds of passes and SYNCHRONISES the stream
// (the table buffer ctx->sat holds its two bit planes); info may be null
int launch_fill_similar(rtdd_ctx *ctx, const rtdd_wand &wand, const PaintTarget &t, rtdd_wand_info *info);
// rtdd_fill_surface: the checked surface wand and the depth map it reads (f32, aligned); three bit planes, otherwise as launch_fill_similar
int launch_fill_surface(rtdd_ctx *ctx, const rtdd_surface_wand &wand, const PaintTarget &t, const float *depth, size_t depthPitch, rtdd_wand_info *info);

// ---- segment.hip --------------------------------------------------------------------------------
// rtdd_segment_surfaces: the checked parameters; t.edited and t.scribble both null or both given, labels and segments may be null;
// SYNCHRONISES (once, or twice), the paint pass is queued behind that
int launch_segment_surfaces(rtdd_ctx *ctx, const rtdd_segmentation &sg, const PaintTarget &t, const float *depth, size_t depthPitch, int32_t *labels,
                            size_t labelsPitch, rtdd_segment *segments, rtdd_segment_info *info);

// ---- effect_kernels.hip -------------------------------------------------------------------------
int launch_effect(rtdd_ctx *ctx, const Effect &e);
// ---- lens_blur.hip: Effect::kLensBlur (called by launch_effect) ------------------------------------
int launch_lens_blur(rtdd_ctx *ctx, const Effect &e);
// ---- relight.hip: Effect::kRelight (called by launch_effect) ---------------------------------------
int launch_relight(rtdd_ctx *ctx, const Effect &e);
// ---- relight_shadow.hip: Effect::kRelightShadow (called by launch_effect) --------------------------
int launch_relight_shadow(rtdd_ctx *ctx, const Effect &e);
// ---- parallax.hip: Effect::kParallax and Effect::kParallaxLayered (called by launch_effect) ---------
int launch_parallax(rtdd_ctx *ctx, const Effect &e);
// ---- ambient_occlusion.hip: Effect::kAmbientOcclusion (called by launch_effect) --------------------
int launch_ambient_occlusion(rtdd_ctx *ctx, const Effect &e);
// ---- lighting.hip: Effect::kLighting (called by launch_effect) -------------------------------------
int launch_lighting(rtdd_ctx *ctx, const Effect &e);
// ---- bokeh.hip: Effect::kBokeh (called by launch_effect) -------------------------------------------
int launch_bokeh(rtdd_ctx *ctx, const Effect &e);
// ---- composite.hip: Effect::kComposite (called by launch_effect) -----------------------------------
int launch_composite(rtdd_ctx *ctx, const Effect &e);
// ---- remove.hip: Effect::kRemove and Effect::kLift (called by launch_effect) -----------------------
// The push-pull's grouping (DESIGN.md section 4 "Remove"), mirrored by REMOVE_TILE, REMOVE_GROUP, REMOVE_APEX and remove_plan() of
// realtimedepthdiffusion_amd/__init__.py: a workgroup owns a kRemoveTile-square tile of a level and takes kRemoveGroup levels in LDS;
// one workgroup takes a level of at most kRemoveApex samples to 1 x 1 and back, its whole chain (at most kRemoveApexChain samples) in LDS.
constexpr int kRemoveTile = 64, kRemoveGroup = 3, kRemoveApex = 8192, kRemoveApexChain = kRemoveApex + kRemoveApex / 2 + 64;
int launch_remove(rtdd_ctx *ctx, const Effect &e);
int launch_lift(rtdd_ctx *ctx, const Effect &e);                   // (Effect::kLiftMatte too)
// ---- mask_distance.hip: Effect::kMaskDistance and Effect::kRefineMask (called by launch_effect) ------
// The distance transform's geometry (DESIGN.md section 4 "Mask distance"), mirrored by EDT_TILE_W, EDT_TILE_H, EDT_BAND, EDT_LDS_REACH
// and mask_distance_plan() of realtimedepthdiffusion_amd/__init__.py: the column pass works on words of kEdtBand rows of a column and
// flags blocks of kEdtTileW columns; a workgroup of the row pass owns kEdtTileW x kEdtTileH pixels, a wave a row of them, and stages its
// row segment with a halo of the reach in LDS up to a reach of kEdtLdsReach (beyond it the neighbours come through the caches).
constexpr int kEdtTileW = 64, kEdtTileH = 4, kEdtBand = 64, kEdtLdsReach = 224, kEdtMaxReach = 1024;
int launch_mask_distance(rtdd_ctx *ctx, const Effect &e);

// ---- cascade.hip -------------------------------------------------------------------------------
int launch_bgr2gray(rtdd_ctx *ctx, const uint8_t *bgr, size_t bp, uint8_t *gray, size_t gp, int rows, int cols);
int launch_pyrdown_u8(rtdd_ctx *ctx, const uint8_t *src, size_t sp, int rows, int cols, uint8_t *dst, size_t dp);
int launch_pyrdown_bgr(rtdd_ctx *ctx, const uint8_t *src, size_t sp, int rows, int cols, uint8_t *dst, size_t dp);     // the same per channel of an interleaved image
struct PyrupBatch { int n = 1; size_t src = 0, dst = 0, edited = 0, mask = 0, coarse = 0; };      // images and byte strides of a batched pyrUp
int launch_pyrup_inject(rtdd_ctx *ctx, const float *src, size_t sp, int rows, int cols, float *dst, size_t dp, int drows, int dcols,
                        const uint8_t *edited, size_t ep, const uint8_t *mask, size_t mp, float *coarse_out = nullptr, size_t cp = 0,
                        int guard_seq = 0 /* != 0: guarded like k_finish, reporting this sequence number */, const PyrupBatch *batch = nullptr);
int launch_depth_to_u8(rtdd_ctx *ctx, const float *src, size_t sp, uint8_t *dst, size_t dp, int rows, int cols);
int launch_decode_annotation(rtdd_ctx *ctx, const uint8_t *bgr, size_t bp, const uint8_t *ann, size_t ap, uint8_t *edited, size_t ep,
                             uint8_t *scribble, size_t sp, int rows, int cols);
int launch_fill_f32(rtdd_ctx *ctx, float *dst, size_t dp, int rows, int cols, float v);
// k_region_codes: the code planes of `n` pyramid levels from one level-0 region pair (edited u8x3, mask u8), one launch over `images`
// images.  Entry i is level shift[i] of the floor chain: rows[i] x cols[i] codes, code (y, x) read at (y << shift, x << shift)
struct RegionLevels {
    static constexpr int kMax = 12;
    int n = 0;
    uint8_t *codes[kMax]; size_t pitch[kMax], stride[kMax];
    int rows[kMax], cols[kMax], shift[kMax], first_block[kMax + 1];
};
int launch_region_codes(rtdd_ctx *ctx, const uint8_t *edited, size_t ep, size_t ze, const uint8_t *mask, size_t mp, size_t zm, RegionLevels &lv, int images);
// ---- pyramid.cpp -------------------------------------------------------------------------------
void pyramid_free(rtdd_ctx *ctx);
// an annotation image is about to be written: one of the pyramid's?  RTDD_ERR_STATE for a level-0 pointer a live frame has retired
// (erases: labels were REMOVED -- when the images are the pyramid's level-0 pair the next estimate rebuilds the coarse levels)
// (the pyramid's own REGION pair, rtdd_pyramid_set_regions: a region change is noted instead, the annotation's state is left alone)
int pyramid_note_write(rtdd_ctx *ctx, const void *scribble, const void *edited, bool erases = false);
int pyramid_check_read(rtdd_ctx *ctx, const void *a, const void *b);     // ... about to be read

// ---- heal.cpp ----------------------------------------------------------------------------------
// persistent kernels (persist_sync.hpp): reserve the launch's flag values and refresh the poll-limit word before a persistent launch;
// read the status word where the stream has just been synchronised (-> RTDD_ERR_TIMEOUT, status cleared)
int prepare_persistent_launch(rtdd_ctx *ctx, int nblocks, int *flag_base);
// in_solve: called from a residual check inside rtdd_solve_ex -- after a successful heal of the calls before it that solve starts over (kRestartSolve)
int check_persistent_status(rtdd_ctx *ctx, bool in_solve = false);
void prune_confirmed(rtdd_ctx *ctx);    // drop the logged calls a copy-back kernel has confirmed (no synchronisation)
int settle_pending(rtdd_ctx *ctx);      // before a call changes what the logged calls ran on: synchronise + check (+ heal) while that state still exists
// the one place a call enters the log: kind, opt and the kind's record filled in by the caller, id assigned here; false: not logged
bool log_call(rtdd_ctx *ctx, PendingOp &op);
// api.cpp: rtdd_solve_ex with everything the library's own callers add to it (c.targets)
int solve_with(rtdd_ctx *ctx, const SolveCall &c, rtdd_solve_info *info, SolveOutcome *out);
// estimate.cpp: an estimate of the pending log again, from the level whose solve has sequence number failed_seq (0: every level)
int estimate_replay(rtdd_ctx *ctx, const PendingOp::Estimate &e, int failed_seq);

// the reference's host-side omega recurrence (src/GPUSolver.cu:282-299)
void omega_schedule(int n, std::vector<float> &out);

}  // namespace rtdd
