/*
 * rtdd.h -- C ABI of librtdd.so, the MI355X-native (gfx950 / HIP) implementation of the
 * RealTimeDepthDiffusion hot path: the Chebyshev-accelerated Jacobi diffusion solve plus the
 * per-pixel edge-weight, annotation and depth-effect passes.
 *
 * This is the drop-in boundary.  Every entry point below replaces one of the reference's ten
 * free functions (file:line given per function, relative to /root/reference); the reference-
 * side binding a maintainer would add is in INTEGRATION.md.  Differences from the reference
 * interface, all deliberate:
 *   - handle based (one rtdd_ctx per GPU, no file-scope globals) so N host threads or N
 *     processes can drive N GPUs; the reference is non-reentrant (src/GPUSolver.cu:13-19);
 *   - every call returns an int status (0 = ok) instead of printf-and-continue
 *     (src/GPUSolver.cu:21-27);
 *   - calls are stream-ordered and ASYNCHRONOUS on the context's stream; the C++ shim that
 *     exports the reference's mangled symbols (csrc/dropin.cpp) adds the device syncs the
 *     reference has (src/GPUSolver.cu:23,314).
 *
 * Pointer semantics are the reference's: every image pointer is a DEVICE pointer to pitched
 * row-major memory, pitch in BYTES next to it, rows/cols in pixels; u8x3 images are
 * interleaved (x*3+c); depth is f32, nominally in [0,255] -- but the solvers' results are the
 * reference's arithmetic, bit for bit, for EVERY f32 depth: negative, huge, infinite or NaN, on
 * free and on Dirichlet pixels (a buffer whose free pixels were never initialised is a legal
 * input).  Only a NaN's sign and payload are left out of that promise, and for such inputs too
 * the result depends on neither the sweep kernel nor the tile.  A u8 image may start at any address
 * and have any pitch that holds a row -- a region of interest of a larger image is a legal
 * argument.  An f32 image (every depth map, and the f32 source and destination of
 * rtdd_convert_to_float, rtdd_pyrup_depth, rtdd_depth_to_u8 and rtdd_index_to_weight) needs a
 * pointer AND a pitch that are multiples of 4: every entry point that takes one returns
 * RTDD_ERR_INVALID otherwise, before anything is launched.  The library never allocates
 * caller-visible memory.  No torch, no C++ types in any signature.
 */
#ifndef RTDD_H
#define RTDD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtdd_ctx rtdd_ctx;
typedef void *rtdd_stream;          /* a hipStream_t; NULL = the device's null stream */

enum rtdd_status {
    RTDD_OK = 0,
    RTDD_ERR_INVALID = 1,           /* bad argument (null pointer, negative size, level out of range ...) */
    RTDD_ERR_STATE = 2,             /* call order violated (solve before allocate / load_weights) */
    RTDD_ERR_HIP = 3,               /* a HIP runtime call failed; see rtdd_last_error() */
    RTDD_ERR_NOMEM = 4,
    RTDD_ERR_NO_DEVICE = 5,         /* no usable gfx950 device: there is NO CPU fallback */
    RTDD_ERR_TIMEOUT = 6            /* a persistent sweep launch gave up waiting for a neighbouring workgroup (the GPU was shared, so
                                       its workgroups were not all resident at once) AND running the affected calls again failed too, or a
                                       wave gave up waiting for a wave of its own workgroup (an internal error).  A first time-out is NOT
                                       an error (the reference's solver always leaves a valid depth map, src/GPUSolver.cu:311-314): the
                                       failed launch and everything queued behind it drain at once, the copy-back kernels behind them store
                                       nothing (every affected call keeps its input), and the next call that synchronises the stream anyway
                                       -- rtdd_ctx_synchronize, rtdd_download, a residual-stopped rtdd_solve_ex -- switches persistent launches
                                       off (suspended for RTDD_OPT_PERSISTENT_REARM_AFTER solves, twice as many after every further time-out,
                                       for good after four: RTDD_OPT_PERSISTENT_SUSPENDED), prints one warning on stderr, runs the solves /
                                       estimates still unconfirmed again from the failed one on and returns RTDD_OK: see RTDD_OPT_TIMEOUT_HEALS.
                                       The three depth effects queued behind an unconfirmed solve are remembered and run again with it (they
                                       may have read the solve's INPUT); the calls that read a solve's output without being remembered --
                                       rtdd_pyrup_depth, rtdd_depth_to_u8, rtdd_index_to_weight, rtdd_upload -- and the calls that change what
                                       a remembered call ran on (rtdd_ctx_set_stream, rtdd_allocate, rtdd_free, rtdd_load_weights,
                                       rtdd_pyramid_create / _destroy / _set_image) first settle the log: synchronise, look at the status
                                       word, heal.  The annotation calls (paint, pyrDown, convert) are neither: they do not depend on a solve.
                                       LIFETIME RULE: the images handed to a solve, an estimate or an effect must stay valid until an rtdd
                                       call that synchronises (rtdd_ctx_synchronize, rtdd_download, rtdd_live_wait, a settling call above) has
                                       returned RTDD_OK -- a replay reads and writes them again, and a hipDeviceSynchronize / hipStreamSynchronize
                                       of the caller's own does not look at the status word.  A call leaves the log as soon as the kernel that
                                       publishes its result has run with the status word clear (no synchronisation needed), so the log holds
                                       calls in flight, not history.  A host that cannot keep that rule sets RTDD_OPT_TIMEOUT_HEAL to 0:
                                       nothing is remembered, a time-out comes back as RTDD_ERR_TIMEOUT from the next synchronising call */
};

/* Solver variants.  RTDD_METHOD_CHEBYSHEV_JACOBI is the reference's only scheme
 * (src/GPUSolver.cu:282-309); the others are extensions with no reference behaviour
 *  and are opt-in through rtdd_solve_ex(). */
enum rtdd_method {
    RTDD_METHOD_CHEBYSHEV_JACOBI = 0,
    RTDD_METHOD_RED_BLACK_GS = 1,
    RTDD_METHOD_MULTIGRID = 2,       /* V(2,2) cycles, operator-dependent interpolation; maxIterations counts CYCLES,
                                      * checkEvery defaults to 1 cycle.  With tolerance > 0 and a check every cycle the driver
                                      * also extrapolates (x + l/(1-l) (x - x_prev)) whenever the residual ratio l of two
                                      * consecutive cycles has settled; tolerance <= 0 runs plain cycles */
    RTDD_METHOD_AUTO = 3             /* to a tolerance (required): V-cycles while they pay (until the tolerance, 60 cycles, or until
                                      * the cycles still needed at the current rate are modelled dearer than the sweeps), then red-black SOR cycles
                                      * (RTDD_RELAXATION_AUTO, started at half length: N = max(rows,cols)/2 rounded up) from there;
                                      * maxIterations caps the SOR sweeps */
};

/* Tunables, rtdd_set_option(ctx, key, value). */
enum rtdd_option {
    RTDD_OPT_FP_CONTRACT = 0,       /* 1 (default): fused multiply-adds where nvcc -fmad=true fuses; 0: none */
    RTDD_OPT_SWEEP_KERNEL = 1,      /* 0 auto (default), 1 one sweep per launch, 2 temporally blocked */
    RTDD_OPT_TEMPORAL_DEPTH = 2,    /* sweeps fused per launch by the blocked kernel (0 = auto) */
    RTDD_OPT_DEFOCUS_PATH = 3,      /* rtdd_simulate_defocus: 0 (default) automatic -- one launch with per-tile summed-area tables in LDS when the largest
                                       nominal window is <= 56 pixels wide (images up to a 2280-pixel diagonal: 1080p), a global table otherwise;
                                       1 the global table always; 2 the tile kernel wherever its region fits (0 falls back to the table for the rest of
                                       the context's life once a call has met depths far outside [0, 255]: windows beyond a tile's region are
                                       summed directly there, exactly but at a cost that grows with their area).  Same bits either way */
    RTDD_OPT_ROWS_PER_WAVE = 4,     /* one-sweep kernel: rows each wave walks (0 = auto) */
    RTDD_OPT_PERSISTENT = 6,        /* (rtdd_get_option returns what is in force: 0 while a time-out has persistent launches suspended)
                                       1 (default): levels whose tiles all fit on the chip at once run ALL sweeps in one launch,
                                       neighbouring workgroups trading halo strips in memory (no kernel boundaries); larger levels (4K, 8K) run
                                       one launch per block of sweeps.  0: one launch per block of sweeps everywhere */
    /* RTDD_METHOD_AUTO prices the V-cycles still needed against finishing with SOR cycles.  The prices are these four CONSTANTS
     * (never a clock: a solve is reproducible); they are options so that the decision can be restated from outside and re-tuned
     * without touching bits by accident.  cycle = FIXED_NS + pixels * CYCLE_FS_PER_PX; sweep = max(FLOOR_NS, pixels * SWEEP_FS_PER_PX). */
    RTDD_OPT_AUTO_CYCLE_FIXED_NS = 9,    /* default 270000 */
    RTDD_OPT_AUTO_CYCLE_FS_PER_PX = 10,  /* default 46000 (femtoseconds per level-0 pixel) */
    RTDD_OPT_AUTO_SWEEP_FS_PER_PX = 11,  /* default 1429 */
    RTDD_OPT_AUTO_SWEEP_FLOOR_NS = 12,   /* default 2500 */
    RTDD_OPT_DEBUG_WITHHOLD_TILE = 7, /* testing aid: tile number + 1 whose hand-off flag a persistent launch never publishes (0 = off),
                                       so that its neighbours run into the poll limit -> RTDD_ERR_TIMEOUT */
    RTDD_OPT_DEBUG_POLL_LIMIT_US = 8, /* testing aid: that poll limit in microseconds (0 = the default, 200 ms) */
    RTDD_OPT_DEBUG_FORCE_STATUS = 13, /* testing aid: value (1, 2) stored into the kernels' status word right behind the next temporally blocked
                                       Jacobi launch, persistent or not, as if a wave of it had given up (one shot: resets to 0); 3 = status 1
                                       now AND once more when that solve is run again, so that the replay fails too (-> RTDD_ERR_TIMEOUT) */
    RTDD_OPT_DEFOCUS_LAST_PATH = 15, /* read only: what the most recent rtdd_simulate_defocus launched -- 1 the global table, 2 the tile kernel (0: none yet).
                                       Setting RTDD_OPT_DEFOCUS_PATH to 0 also forgets an earlier fall-back of the automatic choice to the table */
    RTDD_OPT_TIMEOUT_HEALS = 14,    /* read only: how many times this context has healed a timed-out persistent launch (see RTDD_ERR_TIMEOUT) */
    RTDD_OPT_TIMEOUT_HEAL = 16,     /* 1 (default): heal as described at RTDD_ERR_TIMEOUT; 0: remember nothing, report the time-out */
    RTDD_OPT_PERSISTENT_REARM_AFTER = 17, /* solves run without persistence after the FIRST healed time-out before persistent launches are tried
                                       again (default 64; doubles with every further time-out; after four time-outs persistence stays off;
                                       0: off for good at the first).  Setting RTDD_OPT_PERSISTENT to 1 explicitly re-arms at once */
    RTDD_OPT_PERSISTENT_SUSPENDED = 18, /* read only: 0 persistent launches are armed (or RTDD_OPT_PERSISTENT is 0 by the caller's choice); n > 0: suspended
                                       for n more solves after a time-out; -1: off for the rest of the context's life */
    RTDD_OPT_PENDING_CALLS = 19,    /* read only: calls currently remembered for a replay (see RTDD_ERR_TIMEOUT): those still in flight */
    RTDD_OPT_LIVE_ZERO_COPY = 20,   /* rtdd_live_submit lets the estimate's copy-back kernel store the u8 map straight into hostDepthU8 when that buffer is
                                       page-locked (rtdd_host_alloc, hipHostMalloc, hipHostRegister) -- no staging slot, no download.  1 (default): when
                                       no other frame is in flight (one frame at a time; in a pipelined loop rtdd_live_wait downloads the staged map
                                       while the next frame computes, which is cheaper still); 2: always; 0: never */
    RTDD_OPT_DEFOCUS_STRIPS = 22,   /* the table path of rtdd_simulate_defocus, tile order of the lookup: 0 (default) automatic -- each XCD takes a COLUMN strip of the
                                       image where the table rows between a window's bottom and top edge, over the whole image width, outgrow an XCD's
                                       L2 (from ~4K on: 8K 727 -> 620 us on a smooth depth map, 2.9 -> 1.3 ms with a random depth per pixel, before the corner reuse of the same round), row bands
                                       otherwise; 1 row bands always; 2 column strips always.  Same bits */
    RTDD_OPT_DEFOCUS_LAST_SLICES = 23, /* read only: the horizontal slices the most recent table-path rtdd_simulate_defocus built a table for (1: one
                                       whole-image table: the default) */
    RTDD_OPT_DEFOCUS_SLICE_MB = 24, /* the table path of rtdd_simulate_defocus: a summed-area table (8 bytes per pixel) of more than twice this many MB is
                                       built and looked up slice by slice -- output rows + the tallest nominal window's reach above and below, each slice's
                                       table at most this large and with an origin of its own, all in one buffer.  Default 0: always one whole-image
                                       table (slices measured SLOWER at 8K -- 762 against 725 us: what the 265 MB table loses is L2 reuse, which
                                       RTDD_OPT_DEFOCUS_STRIPS restores, not the Infinity Cache); they are what lets an image beyond 2^29 pixels, whose
                                       whole table would pass 4 GiB, be processed at all.  Same bits either way; depths above 255 (windows beyond a
                                       slice) are answered exactly and send the context's later calls back to the whole-image table */
    RTDD_OPT_ANNOTATION_LDS = 21,   /* 1 (default): an estimate's annotation pyramid walks its levels in LDS (one launch, one memory round trip; pyramids of
                                       up to six levels); 0: the same launch with the levels read back from global memory (a developer's A/B knob) */
    RTDD_OPT_TILE = 5               /* blocked kernel extended tile: 0 auto, 1 = 64x64, 2 = 128x64, 3 = 128x128,
                                       4 = 128x96, 5 = 128x48, 6 = 64x96, 7 = 64x48, 8 = 128x64 (8 px/thread),
                                       9 = 64x64 (4 px/thread), 10 = 64x64 (8 px/thread), 11 = 128x32 (4 px/thread),
                                       12 = 128x96 (16 px/thread, 768 threads), 13 = 128x96 (24 px/thread, 512 threads),
                                       14 = 64x64 in the column layout (1 px x 4 rows per thread; small pyramid levels),
                                       15 = 64x32 and 16 = 64x48 in the column layout */
};

/* ---- context ------------------------------------------------------------------------------- */
int rtdd_ctx_create(int device, rtdd_ctx **out);
int rtdd_ctx_destroy(rtdd_ctx *ctx);
int rtdd_ctx_set_stream(rtdd_ctx *ctx, rtdd_stream stream);
int rtdd_ctx_synchronize(rtdd_ctx *ctx);                 /* hipStreamSynchronize on the context's stream */
int rtdd_set_option(rtdd_ctx *ctx, int key, int value);
int rtdd_get_option(rtdd_ctx *ctx, int key, int *value);
const char *rtdd_last_error(rtdd_ctx *ctx);              /* message of the last failing call on ctx */
const char *rtdd_status_string(int status);
int rtdd_version(void);                                  /* major * 100 + minor.  200: rtdd_solve_info grew from 12 to 36 bytes (kernel .. launches);
                                                          * rtdd_solve_ex / rtdd_refine_depth / rtdd_last_solve_info write the whole struct, so a
                                                          * caller compiled against a 1xx header must be rebuilt (#define RTDD_VERSION below).  210 adds
                                                          * rtdd_pyramid_annotation_changed, RTDD_OPT_TIMEOUT_HEALS and the self-healing time-out; 220: RTDD_OPT_TIMEOUT_HEAL,
                                                          * persistence re-armed after a time-out, rtdd_estimate_depth_batch, RTDD_OPT_LIVE_ZERO_COPY;
                                                          * 230: rtdd_pyramid_level_info, rtdd_live_submit_ex, RTDD_OPT_DEFOCUS_STRIPS / _SLICE_MB / _LAST_SLICES */
#define RTDD_VERSION 230

/* ---- solver (include/GPUSolver.h:6-10) ------------------------------------------------------ */

/* GPUAllocateDeviceMemory(rows, cols, levels) -- src/GPUSolver.cu:33-54.
 * Per-level private scratch for levels 0..levels-1 of size (int)(rows/2^l) x (int)(cols/2^l);
 * sets maxLevel = levels-1 (selects the un-gated weight rule, src/GPUSolver.cu:166,188). */
int rtdd_allocate(rtdd_ctx *ctx, int rows, int cols, int levels);

/* GPUFreeDeviceMemory(levels) -- src/GPUSolver.cu:56-71. */
int rtdd_free(rtdd_ctx *ctx);

/* GPULoadWeights(beta) -- src/GPUSolver.cu:264-272.  LUT w[i] = expf(-beta*i) computed on the
 * HOST with libm like the reference, w[256] = 0, f32 denormals preserved. */
int rtdd_load_weights(rtdd_ctx *ctx, float beta);

/* GPUMatrixFreeSolver(...) -- src/GPUSolver.cu:274-316.  Exactly maxIterations Chebyshev-Jacobi
 * sweeps on level `level`; depth is read (initial guess + Dirichlet values where scribble==255)
 * and overwritten with the result.  beta and tolerance are accepted and ignored, as in the
 * reference (src/GPUSolver.cu:274-275).  rows/cols must not exceed the level's allocation.
 * The bits are the reference's arithmetic for every f32 depth, in range or not (a NaN's sign and
 * payload excepted), whatever RTDD_OPT_SWEEP_KERNEL, RTDD_OPT_TILE and RTDD_OPT_TEMPORAL_DEPTH say:
 * a mean whose weighted sum is +inf or overflows is +inf, clamped to 255, never a NaN clamped to 0. */
int rtdd_matrix_free_solver(rtdd_ctx *ctx, float *depth, size_t depthPitch,
                            const uint8_t *scribble, size_t scribblePitch,
                            const uint8_t *gray, size_t grayPitch,
                            int rows, int cols, float beta, int maxIterations, float tolerance, int level);

/* Extension (no reference counterpart): same inputs, selectable method and an optional
 * residual stop.  With method = CHEBYSHEV_JACOBI, tolerance <= 0 it is bit-identical to
 * rtdd_matrix_free_solver. */
typedef struct rtdd_solve_params {
    int method;                     /* enum rtdd_method */
    int maxIterations;              /* upper bound on sweeps */
    float tolerance;                /* stop when max|J(x)-x| over free pixels <= tolerance; <= 0: never.  A free pixel whose
                                     * |J(x)-x| is NaN counts as +inf: a map with a NaN in it never passes for converged */
    int checkEvery;                 /* residual is evaluated every checkEvery sweeps (0 = 16) */
    float relaxation;               /* RED_BLACK_GS only: SOR factor in (0,2), x <- clamp(x + relaxation (gs - x));
                                     * 0 or 1 = plain Gauss-Seidel; RTDD_RELAXATION_AUTO = SOR cycles.  Cycle c (e = min(c,6)),
                                     * with gap = max(0.005, (2 - min(1.99, 2/(1+sin(4 pi/N)))) / 2^e), N = max(rows,cols):
                                     * N 2^e sweeps at omega = 2 - gap, a quarter as many at max(1, 2 - 10 gap), then <= 100
                                     * plain sweeps with the residual checked every 20 (checkEvery is ignored); cycles repeat
                                     * until tolerance or maxIterations */
} rtdd_solve_params;
#define RTDD_RELAXATION_AUTO (-1.0f)

typedef struct rtdd_solve_info {
    int iterations;                 /* sweeps actually executed (RTDD_METHOD_MULTIGRID: cycles) */
    float residual;                 /* last evaluated max|J(x)-x| (NaN if never evaluated) */
    int cycles;                     /* V-cycles executed (RTDD_METHOD_MULTIGRID, RTDD_METHOD_AUTO), else 0 */
    /* what actually ran, so that a log line identifies the code path (the automatic choices depend on the image size): */
    int kernel;                     /* sweep kernel of the LAST sweep launch: 1 one Jacobi sweep per launch, 2 temporally blocked Jacobi,
                                     * 3 one red-black colour per launch, 4 register-blocked red-black; 0 = no sweep launch */
    int tile;                       /* blocked kernels: tile id (RTDD_OPT_TILE numbering; red-black: 1 = 128x64, 2 = 128x128) */
    int temporal_depth;             /* blocked kernels: sweeps per launch (persistent: per exchange) */
    int persistent;                 /* 1: that launch was persistent (all its sweeps in one launch) */
    int fp_contract;                /* RTDD_OPT_FP_CONTRACT in force */
    int launches;                   /* kernel launches of the solve, k_prepare / k_finish excluded */
} rtdd_solve_info;

int rtdd_solve_ex(rtdd_ctx *ctx, float *depth, size_t depthPitch,
                  const uint8_t *scribble, size_t scribblePitch,
                  const uint8_t *gray, size_t grayPitch,
                  int rows, int cols, int level,
                  const rtdd_solve_params *params, rtdd_solve_info *info);

/* The rtdd_solve_info of the most recent rtdd_solve_ex / rtdd_matrix_free_solver call on this context (also of the per-level
 * solves inside rtdd_estimate_depth: the finest level's). */
int rtdd_last_solve_info(rtdd_ctx *ctx, rtdd_solve_info *info);

/* Read only, for tests and diagnosis: how many waves of this context's persistent Jacobi launches have entered SCALED MODE since the
 * context was created.  A wave in the mode divides every pixel by a uniformly scaled form of the same correctly rounded divide; results
 * are the same bits, and nothing switches the mode off before the launch ends.  In a persistent launch (RTDD_OPT_PERSISTENT) of the tile
 * a 1080p solve runs (tile 4: 128 x 96 pixels, 1024 threads) every wave that may enter the mode enters it before its first sweep, and the count
 * grows by that number of waves with every such launch (each workgroup adds its waves in one step).  In the other persistent tiles a
 * wave enters at the halo exchange behind a block of sweeps that met numerators below 2^-100 -- free pixels enclosed by label-0 strokes
 * decay that far -- and adds 1 there.  The mode is not entered by a wave that holds a pixel with a denormal divisor, nor in a solve whose
 * input holds a depth of 2^32 or more in magnitude, and never by a launch per block of sweeps or a single-tile launch.  Synchronises
 * (rtdd_ctx_synchronize).
 * (A function and not a read-only rtdd_option: found by symbol, no version bump; the next bump of RTDD_VERSION should cover it.) */
int rtdd_scaled_mode_waves(rtdd_ctx *ctx, int *waves);

/* Diagnostic for the parity tests: after a RTDD_METHOD_MULTIGRID solve, copy plane `which` (0-4: couplings E,S,SE,SW and
 * diagonal D; 5-8: interpolation weights; 9-11: e, b, r) of hierarchy level `level` to host memory, dense rows x cols
 * floats.  host == NULL only reports the size.  Synchronises. */
int rtdd_multigrid_level(rtdd_ctx *ctx, int level, int which, float *host, int *rows, int *cols);

/* The edge-weight index pass on its own (loadIndexToWeight, src/GPUSolver.cu:136-224), exposed
 * for parity tests: writes the reference's int2 {left*1000+right, up*1000+down} per pixel,
 * dense (y*cols+x), into a device buffer of rows*cols*2 int32. */
int rtdd_index_to_weight(rtdd_ctx *ctx, const uint8_t *gray, size_t grayPitch,
                         const float *depth, size_t depthPitch,
                         int32_t *index2, int level, int rows, int cols);

/* Colour-guided edge weights (extension; no reference behaviour).  Added after ABI version 230 without a version bump: a host finds
 * rtdd_solve_guided, rtdd_index_to_weight_guided, rtdd_pyrdown_bgr, rtdd_pyramid_set_guide and rtdd_pyramid_guide by symbol, and the next
 * bump of RTDD_VERSION should cover them.
 * The reference reads the photograph through ONE gray channel: the LUT index of the edge between two 4-neighbours p, q is
 * |gray_p - gray_q| (src/GPUSolver.cu:183-222), so a boundary between two colours of equal luminance does not exist for the diffusion.
 * With a BGR guide (interleaved u8x3, pitch >= 3 * cols, any address and any pitch: a region of interest is legal) the index is
 *     index(p, q) = max(|B_p - B_q|, |G_p - G_q|, |R_p - R_q|)
 * an integer in [0, 255] -- a LUT index as it stands, no clamp.  Everything else is loadIndexToWeight's: 256 outside the image, the
 * depth gate of level != maxLevel with its threshold (0 on level 0, 4 otherwise: the index is 0 unless the saturated u8 depths of p and
 * q differ by MORE than it), the saturating u8 cast of the depth.  A BGR guide with B = G = R = v gives the gray guide's indices on v,
 * byte for byte, so such a solve has the reference's bits.  The sweeps never see the guide, only the indices: every method, sweep kernel,
 * tile and launch mode is guided alike.
 * NOTE (a consequence of the reference's gate, not of the guide): on level 0 an edge whose two pixels START at the same u8 depth has index
 * 0 under either guide -- the gate zeroes it before the guide is asked.  A colour edge is found at the coarsest level of an estimate,
 * which is not gated, and inherited by the finer ones through the depth they start from.
 * rtdd_solve_guided with RTDD_GUIDE_GRAY IS rtdd_solve_ex: the same record, the same launches, the same bits.  Its refusals are
 * rtdd_solve_ex's plus an unknown kind (with RTDD_GUIDE_BGR the pitch rule is guidePitch >= 3 * cols).  A healed time-out
 * (RTDD_ERR_TIMEOUT) runs a guided solve again as guided. */
enum rtdd_guide { RTDD_GUIDE_GRAY = 0, RTDD_GUIDE_BGR = 1 };
int rtdd_solve_guided(rtdd_ctx *ctx, float *depth, size_t depthPitch,
                      const uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *guide, size_t guidePitch, int guideKind,
                      int rows, int cols, int level,
                      const rtdd_solve_params *params, rtdd_solve_info *info);
/* rtdd_index_to_weight for either guide: the index pass alone, in the reference's int2 format, for parity tests. */
int rtdd_index_to_weight_guided(rtdd_ctx *ctx, const uint8_t *guide, size_t guidePitch, int guideKind,
                                const float *depth, size_t depthPitch,
                                int32_t *index2, int level, int rows, int cols);

/* Depth regions (extension; no reference behaviour): painted object masks the diffusion cannot cross.  Added after ABI version 230
 * without a version bump: a host finds rtdd_solve_regions, rtdd_index_to_weight_regions, rtdd_region_codes, rtdd_pyramid_set_regions,
 * rtdd_pyramid_regions and rtdd_pyramid_regions_changed by symbol, and the next bump of RTDD_VERSION should cover them together with
 * the colour guide's calls above (and RTDD_IMG_REGION_EDITED / _MASK / _CODE).
 * Where the diffusion may flow is otherwise decided by the photograph alone, and the photograph can be wrong both ways: a weak edge
 * leaks (a step in colour too small to cut is no boundary for the solver, whatever labels are painted), and a texture blocks (a floor
 * of random tiles stops diffusion inside one surface).  A REGION CODE says "this is one object", separately from "this pixel has that
 * depth": one u8 per pixel, 0 = unassigned.
 * THE RULE, for two 4-neighbours p, q inside the image with codes rp, rq.  Let i be the index the existing rule gives -- the gray or
 * BGR guide (above), then the depth gate of level != maxLevel with its threshold.  Nothing about i changes.  Then, in this order:
 *     1. RTDD_REGION_CUT is set and rp != rq               -> the index is 255
 *     2. else RTDD_REGION_SMOOTH is set and rp == rq != 0  -> the index is 0
 *     3. else                                              -> the index is i
 * Outside the image the index stays 256.  THE OVERRIDE COMES AFTER THE GATE: at gated levels the reference zeroes every edge whose two
 * pixels start at the same u8 depth, and a cut holds there too (level 0 of an estimate would otherwise forget it).  An edge between
 * a region and unassigned pixels is cut; an edge between two unassigned pixels is the reference's edge, untouched.
 *   - A cut edge's weight is LUT[255], not 0: 5.6e-45 at the reference's beta 0.4, a denormal.  The per-pixel meta word of the sweeps
 *     has 8 bits per index, so 256 ("no neighbour") cannot be stored there, and the sweep kernels are not touched for it: they read
 *     only those indices, so every method, sweep kernel, tile, launch mode, batch and live path is covered by the prepare pass alone.
 *   - A caller who loads a small beta (rtdd_load_weights) gets a cut as weak as its LUT[255].
 *   - A region with no scribble inside keeps diffusing only within itself, from whatever depth it started with: a region needs a
 *     label of its own.
 *   - A pixel ALL of whose edges are cut has a denormal divisor: the sweep's full-divide path on those pixels (the case
 *     tests/test_gpu_parity.py::test_denormal_divisor_takes_the_full_divide pins).
 * An all-zero code image, or regionFlags 0, or regions == NULL with regionFlags 0, gives the existing indices byte for byte, and the
 * call then IS rtdd_solve_guided: the same record, the same launches, the same bits.  `regions`: u8, pitch >= cols, any address and any
 * pitch (a 4-byte aligned pointer and pitch, next to aligned depth, scribble and guide, take the four-pixel prepare kernel).
 * Refused: what rtdd_solve_guided refuses, unknown flag bits, regions == NULL with regionFlags != 0, a region pitch smaller than a row.
 * A healed time-out (RTDD_ERR_TIMEOUT) runs a region solve again with its regions. */
enum rtdd_region_flags { RTDD_REGION_CUT = 1, RTDD_REGION_SMOOTH = 2 };
int rtdd_solve_regions(rtdd_ctx *ctx, float *depth, size_t depthPitch,
                       const uint8_t *scribble, size_t scribblePitch,
                       const uint8_t *guide, size_t guidePitch, int guideKind,
                       const uint8_t *regions, size_t regionsPitch, int regionFlags,
                       int rows, int cols, int level,
                       const rtdd_solve_params *params, rtdd_solve_info *info);
/* rtdd_index_to_weight_guided with the rule above on top: the index pass alone, in the reference's int2 format, for parity tests. */
int rtdd_index_to_weight_regions(rtdd_ctx *ctx, const uint8_t *guide, size_t guidePitch, int guideKind,
                                 const uint8_t *regions, size_t regionsPitch, int regionFlags,
                                 const float *depth, size_t depthPitch,
                                 int32_t *index2, int level, int rows, int cols);
/* The packing rule of the pyramid's code planes (rtdd_pyramid_set_regions below) on caller images: from a rows x cols level-0 region
 * pair -- `edited` u8x3 and `mask` u8, what the paint calls write -- the codes of pyramid level `level` (0..15), floor(rows / 2^level)
 * x floor(cols / 2^level) of them:
 *     code_level(y, x) = code_0(y << level, x << level),   code_0(y, x) = mask(y, x) == 255 ? edited(y, 3 x) : 0
 * A pixel painted with label 0, or erased, is unassigned.  Top-left sampling composes across levels, so no level depends on another.
 * Stream-ordered; an empty level writes nothing. */
int rtdd_region_codes(rtdd_ctx *ctx, const uint8_t *edited, size_t editedPitch, const uint8_t *mask, size_t maskPitch,
                      int rows, int cols, int level, uint8_t *codes, size_t codesPitch);

/* ---- image processing (include/GPUImageProcessing.h:4-10) ---------------------------------- */

/* GPUConvertToFloat -- src/GPUImageProcessing.cu:8-21,72-79: dst[y][x] = src[y][3x] where mask==255. */
int rtdd_convert_to_float(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, float *dst, size_t dstPitch,
                          const uint8_t *mask, size_t maskPitch, int rows, int cols);

/* GPUPyrDownAnnotation -- src/GPUImageProcessing.cu:23-49,81-91. */
int rtdd_pyrdown_annotation(rtdd_ctx *ctx, const uint8_t *prevScribble, size_t prevScribblePitch,
                            const uint8_t *prevEdited, size_t prevEditedPitch, int previousRows, int previousCols,
                            uint8_t *currScribble, size_t currScribblePitch,
                            uint8_t *currEdited, size_t currEditedPitch, int currentRows, int currentCols);

/* GPUPaintImage -- src/GPUImageProcessing.cu:51-70,93-101 (square brush, integer radius/2).  A NEGATIVE scribbleRadius paints nothing
 * and returns RTDD_OK: the brush's bounding box [x - r/2, x + r/2] is then empty (an accident of the arithmetic, kept because callers may
 * rely on it; the reference's kernel tests the same empty interval).  rtdd_paint_strokes below refuses one instead. */
int rtdd_paint_image(rtdd_ctx *ctx, int x, int y, int scribbleColor, int scribbleRadius,
                     uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch, int rows, int cols);

/* Brush strokes and an eraser (extension; no reference behaviour).  Added after ABI version 230 without a version bump, like the aimed
 * depth effects below: a host finds rtdd_paint_strokes and rtdd_pyramid_annotation_rebuild by symbol.
 * `count` segments in ONE call, applied IN ARRAY ORDER: the last stroke that covers a pixel decides it, as `count` calls one after the
 * other would.  A mouse drag event maps onto one call: the positions since the previous event as a polyline of segments.
 * Coverage of pixel p by a stroke, in exact integer arithmetic, with d = p1 - p0, v = p - p0, h = radius / 2 (C division; `radius` is the
 * reference's scribbleRadius, a DIAMETER):
 *   square: p lies in the Minkowski sum of the segment and [-h, h]^2:  min(x0,x1) - h <= px <= max(x0,x1) + h, the same in y, and
 *           |dx vy - dy vx| <= h (|dx| + |dy|).  For p0 == p1 this is GPUPaintImage's test (src/GPUImageProcessing.cu:59-60).
 *   round:  4 dist^2(p, segment) <= radius^2, without a division: with t = v.d, dd = d.d -- t <= 0: 4 |v|^2 <= radius^2;
 *           t >= dd: 4 |p - p1|^2 <= radius^2; otherwise (2 (dx vy - dy vx))^2 <= radius^2 dd.
 * A painted pixel (label 0..255) gets edited = (label, label, label), scribble = 255, as GPUPaintImage; an erased pixel
 * (label RTDD_STROKE_ERASE) gets edited = original at that pixel, scribble = 0.  Pixels no stroke covers are not written.
 * `strokes` is a HOST array, read before the call returns (the host may reuse it at once); the call is otherwise stream-ordered and
 * asynchronous like rtdd_paint_image.  The kernel runs over the strokes' bounding box only, 256 strokes per launch.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: null strokes with count > 0; count < 0 or count > 4096; the null / pitch /
 * size rules of rtdd_paint_image; rows or cols above 32768; a radius outside [0, 1024]; an unknown brush; a label outside [-1, 255]; an
 * erasing stroke with original == NULL (or an original pitch smaller than a row); an endpoint coordinate outside [-32768, 32767] (the
 * domain the coverage test is exact on).  count == 0 is RTDD_OK and launches nothing.  A retired level-0 pointer of live mode:
 * RTDD_ERR_STATE, as for rtdd_paint_image.
 * On the pyramid's own level-0 RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED pair the call notes the change itself, and asks for
 * rtdd_pyramid_annotation_rebuild when at least one stroke erases. */
enum rtdd_brush { RTDD_BRUSH_SQUARE = 0, RTDD_BRUSH_ROUND = 1 };
#define RTDD_STROKE_ERASE (-1)
typedef struct rtdd_stroke {
    int x0, y0, x1, y1;             /* the segment, pixel coordinates; may lie outside the image; x0 == x1 && y0 == y1: a stamp */
    int radius;                     /* the reference's scribbleRadius (a DIAMETER: half-width radius / 2, C division) */
    int brush;                      /* enum rtdd_brush */
    int label;                      /* 0..255: paint that depth label; RTDD_STROKE_ERASE: remove the annotation */
} rtdd_stroke;
int rtdd_paint_strokes(rtdd_ctx *ctx, const rtdd_stroke *strokes /* HOST array */, int count,
                       uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                       const uint8_t *original, size_t originalPitch, /* may be NULL when no stroke erases */
                       int rows, int cols);

/* Depth-ramp strokes (extension; no reference behaviour; found by symbol like rtdd_paint_strokes, no version bump): a stroke whose label
 * runs linearly from label0 at (x0, y0) to label1 at (x1, y1) -- a floor, a road or a wall seen at an angle in ONE stroke.
 * Everything but the label is rtdd_paint_strokes: the coverage rule of both brushes, array order (the last stroke covering a pixel decides
 * it), a painted pixel gets edited = (L, L, L), scribble = 255, an erased one (label0 == label1 == RTDD_STROKE_ERASE) edited = original,
 * scribble = 0, uncovered pixels are not written; `strokes` is a HOST array read before the call returns; 256 strokes per launch over the
 * strokes' bounding box; on the pyramid's own level-0 pair the call notes the change itself and asks for rtdd_pyramid_annotation_rebuild
 * when a stroke erases; a retired level-0 pointer of live mode: RTDD_ERR_STATE.
 * The label L of a covered pixel p of a painting stroke, with d = p1 - p0, v = p - p0, dd = d.d, in exact integer arithmetic:
 *   dd == 0 (a stamp):  L = label0
 *   otherwise:          t = min(max(v.d, 0), dd)
 *                       N = 2 * (label0 * (dd - t) + label1 * t) + dd          (>= 0)
 *                       L = N / (2 * dd)                                       (C division: round half up; 0 <= L <= 255)
 * i.e. the label at the foot of the perpendicular from p, rounded to nearest, ties up.  Beyond either end of the segment (the caps of a
 * round brush, the corners of a square one) the label is that end's.  The rule is symmetric: (p1, p0, label1, label0) paints the same
 * bytes.  On the documented domain dd < 2^35 inside a stroke's grown box and N < 2^45.  With label0 == label1 the call is
 * rtdd_paint_strokes byte for byte.
 * Refused (RTDD_ERR_INVALID) before any launch, the images untouched: what rtdd_paint_strokes refuses, each of the two labels outside
 * [-1, 255], and exactly ONE of the two labels being RTDD_STROKE_ERASE (an eraser has no ramp). */
typedef struct rtdd_ramp_stroke {
    int x0, y0, x1, y1;             /* as rtdd_stroke */
    int radius, brush;              /* as rtdd_stroke */
    int label0, label1;             /* the label at (x0, y0) and at (x1, y1): both in 0..255, or both RTDD_STROKE_ERASE */
} rtdd_ramp_stroke;
int rtdd_paint_ramp_strokes(rtdd_ctx *ctx, const rtdd_ramp_stroke *strokes /* HOST array */, int count,
                            uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                            const uint8_t *original, size_t originalPitch, /* may be NULL when no stroke erases */
                            int rows, int cols);

/* A mouse drag as ONE continuous ramp: the n points xy[0..2n-1] (x, y, x, y ...) become max(n - 1, 1) records whose labels are spread
 * from label0 at the first point to label1 at the last BY ARC LENGTH.  Host arithmetic only: no context, no launch.
 *   s_0 = 0, s_i = s_(i-1) + sqrt((double)dd_i) accumulated in index order (dd_i the squared length of segment i - 1 .. i), S = s_(n-1);
 *   vertex label l_i = S > 0 ? (int)floor(label0 + (label1 - label0) * (s_i / S) + 0.5) : label0  (doubles; the quotient, the product and
 *   the two sums each rounded on their own, never fused);
 *   segment i gets (l_i, l_(i+1)): neighbouring segments share their vertex label, l_0 == label0, l_(n-1) == label1 when S > 0.
 * n == 1 gives one stamp with both labels label0.  At a joint of a ROUND polyline the later segment's cap repaints up to radius / 2 pixels
 * of the earlier segment's body with the joint's own label (the cap's label is its end's): a deviation of at most the label change over
 * radius / 2 pixels of the earlier segment, on the inner side of the bend.
 * RTDD_ERR_INVALID: null xy or out; n < 1 or n > 4097; a coordinate, radius or brush rtdd_paint_ramp_strokes would refuse; a label outside
 * [0, 255] (RTDD_STROKE_ERASE too: an eraser has no ramp). */
int rtdd_ramp_polyline(const int *xy /* n points: x, y, x, y ... */, int n, int radius, int brush,
                       int label0, int label1, rtdd_ramp_stroke *out /* max(n - 1, 1) records */);

/* A filled polygon -- the lasso (extension; no reference behaviour; found by symbol like rtdd_paint_ramp_strokes, no version bump; the next
 * bump of RTDD_VERSION should cover rtdd_paint_strokes, rtdd_pyramid_annotation_rebuild, rtdd_paint_ramp_strokes, rtdd_ramp_polyline and
 * rtdd_fill_polygon): a region outlined by the user gets one label ("all of this is at that depth"), a ramp ("all of this is that
 * plane") or is erased ("forget everything I drew in here").  All of it exact integer arithmetic.
 * Contour: the closed contour v_0 .. v_(n-1), v_0 of the n vertices xy = x, y, x, y ... -- integer pixel coordinates, which may lie
 *   outside the image; the contour may intersect itself and may repeat a vertex.
 * Winding of pixel p = (px, py): w = 0; for every edge a -> b of the contour
 *   cr = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
 *   w += 1 when ay <= py < by and cr > 0
 *   w -= 1 when by <= py < ay and cr < 0
 *   (a horizontal edge never counts).
 * Boundary: p lies on an edge when cr == 0, min(ax,bx) <= px <= max(ax,bx) and min(ay,by) <= py <= max(ay,by).
 * Coverage: p is covered when it lies on the boundary, or when w != 0 (RTDD_FILL_NONZERO), or when w is odd (RTDD_FILL_EVEN_ODD).  The
 *   region is closed: every vertex inside the image is covered; the covered set does not depend on the contour's direction (reversal
 *   negates w) or on which vertex comes first; a contour with n = 1 or n = 2, or with all vertices collinear, covers exactly the lattice
 *   points of its segments.
 * Label: rtdd_paint_ramp_strokes' L with the axis (ax0, ay0) - (ax1, ay1) as the segment: with d = a1 - a0, v = p - a0, dd = d.d,
 *   dd == 0 or label0 == label1:  L = label0
 *   otherwise:                    t = min(max(v.d, 0), dd)
 *                                 N = 2 * (label0 * (dd - t) + label1 * t) + dd
 *                                 L = N / (2 * dd)                             (C division: round half up; 0 <= L <= 255)
 *   Beyond either end of the axis the label is that end's.  Any plane over the region can be expressed: lay the axis along its gradient.
 * Writes: painting (labels 0..255) writes edited = (L, L, L), scribble = 255; erasing (both labels RTDD_STROKE_ERASE) writes edited =
 *   original at that pixel, scribble = 0; uncovered pixels are not written.
 * Domain: vertex and axis coordinates in [-32768, 32767]; rows and cols at most 32768; 1 <= n <= 768 (n == 0: RTDD_OK, nothing launched).
 *   On it |cr| < 2^34, dd < 2^35, N < 2^45 and |w| <= 384.  The vertices travel as kernel arguments (4 bytes each): a host with a longer
 *   lasso thins it out.
 * Refused (RTDD_ERR_INVALID) before any launch, the images untouched: a null fill; a null xy with n > 0; n outside [0, 768]; an unknown
 *   rule; a vertex or axis coordinate outside the domain; a label outside [-1, 255]; exactly ONE label being RTDD_STROKE_ERASE; erasing
 *   with original == NULL or an original pitch smaller than a row; the null, pitch and size rules of rtdd_paint_strokes.  A retired
 *   level-0 pointer of live mode: RTDD_ERR_STATE.
 * On the pyramid's own level-0 RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED pair the call notes the change itself, and asks for
 * rtdd_pyramid_annotation_rebuild when it erases, exactly as rtdd_paint_strokes.  xy and fill are HOST memory, read before the call
 * returns; the call is otherwise stream-ordered and asynchronous: ONE launch over the contour's bounding box clipped to the image (none for
 * a contour wholly outside).  Calls compose by stream order with each other and with the stroke calls: the later call decides a pixel. */
enum rtdd_fill_rule { RTDD_FILL_NONZERO = 0, RTDD_FILL_EVEN_ODD = 1 };
typedef struct rtdd_fill {
    int rule;                   /* enum rtdd_fill_rule */
    int ax0, ay0, ax1, ay1;     /* the ramp's axis: label0 at (ax0, ay0), label1 at (ax1, ay1); ignored when label0 == label1 */
    int label0, label1;         /* both in 0..255, or both RTDD_STROKE_ERASE */
} rtdd_fill;
int rtdd_fill_polygon(rtdd_ctx *ctx, const int *xy /* HOST: n vertices x, y, x, y ... */, int n, const rtdd_fill *fill,
                      uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *original, size_t originalPitch, /* may be NULL unless erasing */
                      int rows, int cols);

/* Fill what looks like the clicked pixel -- the magic wand (extension; no reference behaviour; found by symbol like rtdd_fill_polygon, no
 * version bump; the next bump of RTDD_VERSION should cover rtdd_fill_similar too): one click inside a surface selects everything joined to
 * the click whose colour is close to the clicked colour, and the selection gets rtdd_fill_polygon's label, ramp or erasure.  All of it
 * exact integer arithmetic; the covered set is a connected component, so the bytes do not depend on how the device schedules the search.
 * Seed colour: (sB, sG, sR) = original at (x, y), READ ON THE DEVICE when the call runs.
 * Eligible: pixel p with colour (B, G, R) in `original` is eligible when max(|B - sB|, |G - sG|, |R - sR|) <= tolerance -- the Chebyshev
 *   distance RTDD_GUIDE_BGR takes its index from; a gray image passed as B = G = R behaves as gray.  The seed is always eligible;
 *   tolerance 255 makes every pixel eligible.
 * Covered: with RTDD_WAND_GLOBAL every eligible pixel.  Otherwise the eligible pixels joined to the seed by a path of eligible pixels
 *   whose steps go to one of the 4 neighbours (left, right, up, down) or, with RTDD_WAND_CONNECT_8, to one of the 8 neighbours.  The image
 *   border ends a path: nothing wraps.  At least the seed is covered.
 * What "similar" reads: `original` only.  The scribbles and labels already in the pair play no part in it.
 * Label and writes: rtdd_fill_polygon's.  With d = a1 - a0, v = p - a0, dd = d.d along the axis (ax0, ay0) - (ax1, ay1),
 *   dd == 0 or label0 == label1:  L = label0
 *   otherwise:                    t = min(max(v.d, 0), dd);  N = 2 * (label0 * (dd - t) + label1 * t) + dd;  L = N / (2 * dd)
 *   painting (labels 0..255) writes edited = (L, L, L), scribble = 255; erasing (both labels RTDD_STROKE_ERASE) writes edited = original
 *   at that pixel, scribble = 0; uncovered pixels are not written.
 * The limit of the tool: a boundary whose step in colour is within the tolerance is no boundary.  An object of gray 100 on gray 108, both
 *   with noise of +-2, selected with tolerance 5 leaks into the background (102 against 106); with a step of 12 the selection is exactly
 *   the object.  Choose the tolerance below the weakest edge of the region.
 * Refused (RTDD_ERR_INVALID) before any launch, the images untouched: a null wand; a seed outside the image; a tolerance outside [0, 255];
 *   flag bits other than the two below; an axis coordinate outside [-32768, 32767]; a label outside [-1, 255]; exactly ONE label being
 *   RTDD_STROKE_ERASE; the null, pitch and size rules of rtdd_fill_polygon (rows or cols above 32768 among them); a null original or an
 *   original pitch smaller than a row -- ALWAYS here, not only when erasing: it is what "similar" reads.  rows == 0 or cols == 0 is
 *   RTDD_ERR_INVALID too, unlike the other paint calls: no seed lies inside an empty image.  A retired level-0 pointer of live mode:
 *   RTDD_ERR_STATE.
 * On the pyramid's own level-0 RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED pair the call notes the change itself, and asks for
 * rtdd_pyramid_annotation_rebuild when it erases, exactly as rtdd_fill_polygon.
 * THE CALL SYNCHRONISES, unlike the other paint calls: the search grows the selection in passes over the image, and how many it needs
 * depends on the data, so the host reads a counter back between rounds of passes.  It returns with both images written and `info` filled.
 * Work queued on the context's stream in front of it is waited for; logged solves and estimates are confirmed (or healed) first, as by
 * rtdd_index_to_weight_guided.  The cost is a handful of nearly empty launches per 64 pixels of distance the selection travels, plus one
 * synchronisation per round of 8 passes.  info->passes counts the passes up to the first that changed nothing: a diagnostic, NOT
 * deterministic (a pass may or may not see what a neighbouring wave wrote in the same pass); everything else is. */
enum rtdd_wand_flags { RTDD_WAND_CONNECT_8 = 1,   /* default: 4-connected */
                       RTDD_WAND_GLOBAL    = 2 }; /* every similar pixel of the image, connected or not */
typedef struct rtdd_wand {
    int x, y;                   /* the clicked pixel; must lie inside the image */
    int tolerance;              /* 0..255 */
    int flags;                  /* enum rtdd_wand_flags, or-ed */
    int ax0, ay0, ax1, ay1;     /* the ramp's axis, as rtdd_fill */
    int label0, label1;         /* both 0..255, or both RTDD_STROKE_ERASE */
} rtdd_wand;
typedef struct rtdd_wand_info {
    int pixels;                 /* covered pixels (>= 1) */
    int x0, y0, x1, y1;         /* their inclusive bounding box */
    int passes;                 /* grow passes that ran: a diagnostic, NOT deterministic (0 with RTDD_WAND_GLOBAL) */
} rtdd_wand_info;
int rtdd_fill_similar(rtdd_ctx *ctx, const rtdd_wand *wand,
                      uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *original, size_t originalPitch,   /* always needed: it is what "similar" reads */
                      int rows, int cols, rtdd_wand_info *info /* may be NULL */);

/* Fill the surface under the clicked pixel -- the wand that follows the depth map, not colour (extension; no reference behaviour; found by
 * symbol like rtdd_fill_similar, no version bump; the next bump of RTDD_VERSION should cover rtdd_fill_surface too): one click on an object
 * selects "the thing at this distance, bounded by depth discontinuities", or, globally, "everything in this band of depths", and the
 * selection gets rtdd_fill_polygon's label, ramp or erasure.  Every comparison below is on f32 values, each operation rounded once.
 * Clamped depth: d'(p) = d > 0 ? fminf(d, 255) : +0 for the depth d at p -- rtdd_remove_object's rule: a NaN, -0 and every negative depth
 *   are +0, +inf is 255, a denormal stays what it is.
 * Seed depth: ds = d'(x, y), READ ON THE DEVICE when the call runs.
 * Band: lo = ds - below, hi = ds + above (one f32 operation each).
 * Admissible: p is admissible iff lo <= d'(p) && d'(p) <= hi.  The seed always is; 255 on a side is no limit on that side.
 * Link: two 4-neighbours p, q inside the image are linked iff both are admissible and fabsf(d'(p) - d'(q)) <= step (one f32 subtraction;
 *   symmetric, since a - b == -(b - a) exactly).
 * Covered: the pixels joined to the seed by a path of links; at least the seed.  The image border ends a path: nothing wraps.  With
 *   RTDD_SURFACE_GLOBAL every admissible pixel is covered, linked or not; `step` is validated and otherwise ignored.
 * Connectivity: 4-neighbours only.  A link is a property of a pair of pixels, kept as one bit plane per direction; diagonal links would
 *   take two more link planes and are not built.
 * The covered set is a connected component of an undirected graph: the bytes do not depend on how the device schedules the search.
 * Label and writes: exactly rtdd_fill_polygon's -- the constant label, the ramp along the axis (ax0, ay0) - (ax1, ay1), or the erasure;
 *   uncovered pixels are not written.  `depth` is never written.
 * What the tool reads: `depth` only -- neither the colours nor the labels already in the pair.  Where it fails:
 *   - a surface that touches another at the same depth, such as an object's foot on a floor, is joined to it; the band (below, above) is
 *     what stops the floor from running away;
 *   - a selection is only as good as the depth map.  A 48 x 40 ellipse of 513 pixels in three parts of gray 30 / 120 / 230 on gray 170
 *     (noise +-2), one stroke of label 60 across the parts, one stamp of 200 on the background, solved for 300 or 1000 sweeps: the depth
 *     is 60.0 on every object pixel and at least 132.4 outside, and step 1, 2, 4 or 8 (or the band 30 with step 255, or the global band)
 *     selects exactly the 513 pixels -- no tolerance of rtdd_fill_similar does (it misses 301 or takes 1407 of the background).  The same
 *     ellipse filled with 2 x 2 tiles of random grays 60..140 blocks the single-level solve inside the object: the depth there ranges
 *     from 60 to 128 and the rule covers 84 to 150 of the 513 pixels (steps 2..8, 300 to 3000 sweeps), none of the background.
 *     RTDD_REGION_SMOOTH exists for that case.
 * Not built: 8-connectivity; a rule that reads colour AND depth; re-estimating after the click (the caller's to queue).
 * Refused (RTDD_ERR_INVALID) before any launch, the images untouched: a null wand; a null depth; a depth pitch smaller than 4 * cols or
 *   not a multiple of 4; a depth pointer not 4-byte aligned; a seed outside the image (rows == 0 or cols == 0 included: no seed lies inside
 *   an empty image); step, below or above non-finite or outside [0, 255]; flag bits other than RTDD_SURFACE_GLOBAL; an axis coordinate
 *   outside [-32768, 32767]; a label outside [-1, 255]; exactly ONE label being RTDD_STROKE_ERASE; the null, pitch and size rules of
 *   rtdd_fill_polygon -- `original` may be NULL unless erasing.  A retired level-0 pointer of live mode: RTDD_ERR_STATE.
 * On the pyramid's own level-0 RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED pair the call notes the change itself, and asks for
 * rtdd_pyramid_annotation_rebuild when it erases, exactly as rtdd_fill_similar.  The region pair (RTDD_IMG_REGION_EDITED / _MASK) is a
 * legal target, and the intended one for rtdd_remove_object, rtdd_lift_layer and a background plate.
 * THE CALL SYNCHRONISES, like rtdd_fill_similar and for the same reason.  Logged solves and estimates are confirmed (or healed) first:
 * `depth` is usually the output of an estimate that is still in the log, and it is final before it is read.  info->passes is a
 * diagnostic, NOT deterministic, and 0 with RTDD_SURFACE_GLOBAL; everything else is deterministic. */
enum rtdd_surface_flags { RTDD_SURFACE_GLOBAL = 1 };   /* every admissible pixel, connected or not */
typedef struct rtdd_surface_wand {
    int   x, y;                 /* the clicked pixel; inside the image */
    float step;                 /* finite, [0, 255]: two neighbours are joined when their depths differ by at most this */
    float below, above;         /* finite, [0, 255]: only depths in [ds - below, ds + above] take part; 255 = no limit on that side */
    int   flags;                /* enum rtdd_surface_flags */
    int   ax0, ay0, ax1, ay1;   /* the ramp's axis, as rtdd_fill */
    int   label0, label1;       /* both 0..255, or both RTDD_STROKE_ERASE */
} rtdd_surface_wand;
int rtdd_fill_surface(rtdd_ctx *ctx, const rtdd_surface_wand *wand,
                      uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *original, size_t originalPitch,   /* may be NULL unless erasing */
                      const float *depth, size_t depthPitch,           /* DEVICE f32, read only */
                      int rows, int cols, rtdd_wand_info *info /* may be NULL */);

/* Every surface of the depth map in one call -- connected-component labelling of rtdd_fill_surface's link graph (extension; no reference
 * behaviour; found by symbol like rtdd_fill_surface, no version bump; the next bump of RTDD_VERSION should cover it too).  Where the wand
 * answers "what is under this click", this answers "what are the surfaces": the largest components are numbered and painted as region
 * codes, and a label map turns every later click into a lookup.  Every comparison is on f32 values, each operation rounded once.
 * Clamped depth: d'(p) = d > 0 ? fminf(d, 255) : +0 -- rtdd_fill_surface's: a NaN, -0 and every negative depth are +0, +inf is 255.
 * Admissible: lo <= d'(p) && d'(p) <= hi, with lo and hi given as absolute values: there is no seed, nothing is read to form the band.
 * Link: two 4-neighbours p, q inside the image are linked iff both are admissible and fabsf(d'(p) - d'(q)) <= step (one f32
 *   subtraction): exactly rtdd_fill_surface's link.
 * Component: the pixels joined by a path of links.  An admissible pixel with no link is a component of one pixel; an inadmissible pixel
 *   belongs to no component.  The image border ends a path.
 * Root: the smallest linear index y * cols + x of a component's pixels.  Size: the number of its pixels.
 * Candidates: the components of at least minPixels pixels.
 * Ranking: candidates by size descending, then by root ascending.  The first K = min(candidates, maxRegions) are the regions; region k
 *   (0-based) has the code firstCode + k.
 * Writes, on the paint calls' pair (edited u8 x 3, scribble u8): a pixel of region k gets edited = (code, code, code), scribble = 255;
 *   every other pixel is not written.  `depth` is never written.  The region pair (RTDD_IMG_REGION_EDITED / _MASK) is the intended target
 *   and the annotation pair is legal; on the pyramid's own pairs the call notes the change exactly as rtdd_fill_surface.  edited and
 *   scribble may BOTH be NULL when only the label map or the records are wanted.
 * Label map (optional): device int32, pitch a multiple of 4 and at least 4 * cols, pointer 4-byte aligned.  Every pixel is written exactly
 *   once: the root of its component, or -1 where it is inadmissible.  The padding keeps its bytes.
 * Records (optional): a HOST array of maxRegions entries; the first K are filled, in rank order: the code, the size, the root as
 *   (rootX, rootY), the inclusive bounding box, and dmin / dmax, the smallest and largest d' of the region (d' >= +0, so the order of the
 *   bit patterns is the order of the values: integer minima and maxima of the bits, exact; nothing is summed).
 * Info: components (all of them), candidates, regions (K) and pixels (the sum over the regions).  Everything returned is deterministic: the
 *   result is a property of an undirected graph.  There is no `passes`: nothing iterates to a fixpoint.
 * Refused (RTDD_ERR_INVALID) before any launch, nothing written: a null parameter struct; a null depth; a depth pitch smaller than
 *   4 * cols or not a multiple of 4, a depth pointer not 4-byte aligned; step, lo or hi non-finite or outside [0, 255]; lo > hi;
 *   minPixels < 1; maxRegions outside 1..255; firstCode outside 1..255 or firstCode + maxRegions - 1 > 255; any flag bit (none is defined);
 *   rows or cols of 0, negative or above 32768; exactly ONE of edited and scribble being NULL; a pitch of the pair smaller than a row; a
 *   label map whose pitch or pointer breaks the rule above.  A retired level-0 pointer of live mode: RTDD_ERR_STATE.  Scratch that cannot
 *   be allocated: RTDD_ERR_NOMEM, nothing written.
 * THE CALL SYNCHRONISES, because it returns counts and records: once, or twice when more than 1024 components have minPixels pixels (the
 * candidates beyond the first 1024 take a second copy).  Logged solves and estimates are confirmed (or healed) first, as by
 * rtdd_fill_surface.  The label map is complete when the call returns; the writes to the pair are queued on the context's stream behind
 * it, like every other paint call's.  Not logged by the heal log.  Six launches (five without a pair), whatever the data and the size:
 * links, tile labels, border merge, flatten and reduce, collect, paint.  The scratch is the context's table buffer: about 17 bytes per
 * pixel for the planes and the parents, 28 per pixel for the records and 32 * rows * cols / minPixels for the candidate list.
 * Not built: 8-connectivity; a rule over colour and depth; merging small components into neighbours; clearing the rest of the pair;
 * numbering by nearness (the records carry dmin: renumber on the host). */
typedef struct rtdd_segmentation {
    float step;                 /* finite, [0, 255]: rtdd_surface_wand's */
    float lo, hi;               /* finite, [0, 255], lo <= hi: only depths in [lo, hi] take part */
    int   minPixels;            /* >= 1: smaller components are no candidates */
    int   maxRegions;           /* 1..255 */
    int   firstCode;            /* 1..255, firstCode + maxRegions - 1 <= 255 */
    int   flags;                /* 0 */
} rtdd_segmentation;
typedef struct rtdd_segment {
    int   code, pixels, rootX, rootY;
    int   x0, y0, x1, y1;       /* inclusive bounding box */
    float dmin, dmax;           /* smallest and largest clamped depth */
} rtdd_segment;                 /* 40 bytes */
typedef struct rtdd_segment_info { int components, candidates, regions, pixels; } rtdd_segment_info;
int rtdd_segment_surfaces(rtdd_ctx *ctx, const rtdd_segmentation *seg,
                          uint8_t *edited, size_t editedPitch, uint8_t *scribble, size_t scribblePitch,   /* both NULL: nothing painted */
                          const float *depth, size_t depthPitch,           /* DEVICE f32, read only */
                          int32_t *labels, size_t labelsPitch,             /* DEVICE int32, may be NULL */
                          int rows, int cols, rtdd_segment *segments /* HOST, maxRegions entries, may be NULL */,
                          rtdd_segment_info *info /* may be NULL */);

/* ---- depth effects (include/GPUDepthEffect.h:4-9) ------------------------------------------ */

/* GPUSimulateDefocus -- src/GPUDepthEffect.cu:29-72,105-113 (exact, via an integer summed-area table). */
int rtdd_simulate_defocus(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                          const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                          int rows, int cols);

/* GPUSimulateDesaturation -- src/GPUDepthEffect.cu:8-27,95-103. */
int rtdd_simulate_desaturation(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                               const uint8_t *gray, size_t grayPitch, const float *depth, size_t depthPitch,
                               uint8_t *artistic, size_t artisticPitch, int rows, int cols);

/* GPUSimulateHaze -- src/GPUDepthEffect.cu:74-93,115-123. */
int rtdd_simulate_haze(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                       const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                       int rows, int cols);

/* ---- aimed depth effects (extensions; no reference behaviour) --------------------------------
 * Added after ABI version 230 without a version bump: a host finds them by symbol (dlsym).  The next bump of RTDD_VERSION
 * should cover them (rtdd_simulate_refocus, rtdd_simulate_lens_blur, rtdd_simulate_haze_ex, rtdd_simulate_stereo, rtdd_simulate_relight,
 * rtdd_simulate_relight_shadowed, rtdd_simulate_parallax, rtdd_simulate_ambient_occlusion, rtdd_simulate_lighting, rtdd_simulate_bokeh,
 * rtdd_composite_layer, rtdd_remove_object, rtdd_lift_layer, rtdd_simulate_parallax_layered),
 * together with a
 * parameterised live effect
 * (rtdd_live_submit_ex takes an effect code only and knows none of them). */

/* Refocus: the defocus effect sharp at a chosen depth instead of at depth 0.
 *   K = (int)(aperture * sqrtf(rows*rows + cols*cols))   -- double times float, truncated, as GPUDepthEffect.cu:42; aperture 0.025 gives
 *                                                           the reference's K.  Computed on the host.
 *   f = focusDepth when focusX < 0; otherwise the depth map's value at (focusX, focusY), READ BY THE KERNEL ON THE DEVICE when it runs
 *       (no host synchronisation: the call may sit behind an asynchronous estimate, and "focus on what I clicked" follows the map).
 *   per pixel: dist = fabsf(d - f) in f32, k = (int)(K * dist / 255.0), half-width k/2, the box [y - k/2, y + k/2) x [x - k/2, x + k/2)
 *   clipped to the image, (uchar)(sum / count) per channel in f32, the original pixel when count == 0 -- GPUDepthEffect.cu:43-70
 *   with dist in place of depth.
 * Identity: refocus(orig, d, f, aperture 0.025) == rtdd_simulate_defocus on the map fabsf(d - f), bit for bit; f = 0 on a map with
 * every d in [0, 255] is rtdd_simulate_defocus itself.  Same paths, options and fall-backs as rtdd_simulate_defocus
 * (RTDD_OPT_DEFOCUS_PATH / _STRIPS / _SLICE_MB; RTDD_OPT_DEFOCUS_LAST_PATH reports the path).
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size, in
 * place); a negative or non-finite aperture; K > 255 (then every window of a depth map has count <= 254^2 < 2^16 and channel sums
 * < 2^24: the domains the exact integer sums and quotients are proven on -- the default K is 220 at 8K, and at 1080p the cap allows
 * about 4.6 x the default blur); a non-finite focusDepth when it is used; a focus pixel outside the image when focusX >= 0. */
int rtdd_simulate_refocus(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                          const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                          int rows, int cols, double aperture, float focusDepth, int focusX, int focusY);

/* Lens blur: refocus through a round aperture -- the window is a disc instead of a box, so out-of-focus highlights come out round.
 *   K, f and the focus-pixel form are rtdd_simulate_refocus's, K computed on the host, the focus pixel read by the kernel when it runs.
 *   shape RTDD_APERTURE_BOX: rtdd_simulate_refocus itself, bit for bit (the same kernels).
 *   shape RTDD_APERTURE_DISC, per pixel (x, y): dist = fabsf(d - f) in f32, kf = (double)((float)K * dist) / 255.0, k = 0 when kf is NaN or
 *   <= 0, 255 when kf >= 255, else (int)kf (for a depth map in [0, 255] the clamp never acts: it makes the effect total and bounded --
 *   the disc has no fall-back path and sets no sticky state); the window is the image's pixels (px, py) with
 *   4 * ((px - x)^2 + (py - y)^2) <= k * k, a disc of diameter k inscribed in the box's k x k -- rows dy with 4 dy^2 <= k^2, in each the
 *   span x - w .. x + w, w = isqrt((k*k - 4*dy*dy) / 4), clipped to the image.  The centre always belongs (count >= 1); per channel
 *   out = (uchar)(sum / count) in f32; k <= 1 gives the original pixel.  count <= 51 101 < 2^16 and the sums are < 2^24: exact.
 * RTDD_OPT_DEFOCUS_PATH selects the disc's path as the box's (0 automatic, 1 a global table of row prefixes, 2 the tile kernel where its
 * region fits: K / 2 <= 28); RTDD_OPT_DEFOCUS_LAST_PATH reports it.  The output does not depend on RTDD_OPT_FP_CONTRACT.  Deterministic.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: everything rtdd_simulate_refocus refuses (K > 255 included); a shape
 * other than the two; original == artistic (not in place). */
enum rtdd_aperture_shape { RTDD_APERTURE_BOX = 0, RTDD_APERTURE_DISC = 1 };
int rtdd_simulate_lens_blur(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                            const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                            int rows, int cols, double aperture, float focusDepth, int focusX, int focusY, int shape);

/* Bokeh: the occlusion-aware lens blur.  rtdd_simulate_lens_blur is a gather: the OUTPUT pixel sizes the window from its own depth, so a
 * blurred background averages a sharp foreground subject's colours in (a halo), and a blurred foreground keeps a hard silhouette.  Here
 * every SOURCE pixel spreads its colour over its own circle of confusion, and a source behind the target spreads no wider than the
 * target's own circle.  Evaluated as a gather; all arithmetic after step 2 is integer, so the sums do not depend on their order.
 *   1. K = (int)(aperture * sqrtf(rows*rows + cols*cols)) on the host, as rtdd_simulate_refocus's.  f0 = focusDepth when focusX < 0;
 *      otherwise the depth map's value at (focusX, focusY), READ BY THE KERNEL ON THE DEVICE when it runs (no host synchronisation, as
 *      refocus's focus).  f = fminf(fmaxf(f0, 0), 255), a NaN giving 0 (stereo's clamp).
 *   2. per pixel q, the signed circle of confusion: d' = fminf(fmaxf(d, 0), 255) (a NaN depth is 0), t = d' - f in f32,
 *      kf = (double)((float)K * fabsf(t)) / 255.0, k = (int)kf (in [0, K]: |t| <= 255), s = t < 0 ? -k : k.  For a map within [0, 255]
 *      k is RTDD_APERTURE_DISC's diameter.
 *   3. source q and target p, both inside the image: ke = (s_q > s_p) ? min(k_q, k_p) : k_q -- a source behind the target spreads no
 *      wider than the target's own circle; q reaches p iff 4 * ((qx - px)^2 + (qy - py)^2) <= ke * ke, the disc test of
 *      RTDD_APERTURE_DISC.  p always reaches itself.
 *   4. wt[k] = floor(2^30 / N(k)) for k = 0 .. 127, N(k) the number of integer (dx, dy) with 4 (dx^2 + dy^2) <= k^2 (N(0) = N(1) = 1,
 *      N(127) = 12645, wt[127] = 84914).  W = the sum of wt[ke] over the sources that reach p, S_c = the sum of wt[ke] * o_c(q) over the
 *      same sources, out_c = floor(S_c / W) per channel c of B, G, R.  W >= wt[127] > 0; at most 127^2 sources reach p, so
 *      S_c < 2^14 * 2^30 * 2^8 = 2^52: exact in 64 bits.
 * Identities: on a map whose every pixel has the same s the output is rtdd_simulate_lens_blur(..., RTDD_APERTURE_DISC) byte for byte
 * (floor(wt * sum / (wt * n)) = floor(sum / n), and with n <= 12645 the f32 (uchar)(sum / count) cannot round up to the next integer);
 * where every k <= 1 the output is the original; a pixel with s_p = 0 on a map that has no s < 0 anywhere keeps its original bytes.
 * Deterministic; the output does not depend on RTDD_OPT_FP_CONTRACT; no fall-back path, no sticky state.  One kernel launch.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: everything rtdd_simulate_lens_blur refuses (original == artistic
 * included); K > 127, so that s fits 8 bits and a tile with its halo fits the LDS.  The default aperture gives K = 55 at 1080p and 110 at
 * 4K; at 8K it gives 220, which is refused: 8K needs an aperture of 0.0144 or less (K = 126). */
int rtdd_simulate_bokeh(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                        const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                        int rows, int cols, double aperture, float focusDepth, int focusX, int focusY);

/* Haze with a density and an airlight colour (GPUDepthEffect.cu:74-93 with its constants as parameters):
 *   t = exp((float)((double)(-beta * d) / 255.0)) by the same deterministic exp as rtdd_simulate_haze,
 *   per channel c of B, G, R: out = (uchar)(t * o + (1 - t) * air_c) in f32, fused or not per RTDD_OPT_FP_CONTRACT as in
 *   rtdd_simulate_haze.  beta = 2 with air (255, 255, 255) gives rtdd_simulate_haze's bytes.
 * beta must be finite and in [0, 64] (else RTDD_ERR_INVALID); the other rules are the three effects'. */
int rtdd_simulate_haze_ex(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                          const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                          int rows, int cols, float beta, uint8_t airB, uint8_t airG, uint8_t airR);

/* Stereo: a second eye's view rendered from the depth map (0 near, 255 far, as haze reads it), or a red-cyan anaglyph.  Each row on
 * its own; D = disparity:
 *   d' = fminf(fmaxf(d, 0), 255) (a NaN depth is 0);  z0 = zeroParallaxDepth when zeroX < 0, otherwise the depth map's value at
 *       (zeroX, zeroY), clamped alike and READ BY THE KERNEL ON THE DEVICE when it runs (no host synchronisation, as refocus's focus);
 *   s(x) = (int)rintf(((float)D * (d' - z0)) / 255.0f), each operation rounded in f32, none fused, rintf half to even: |s| <= |D|;
 *   source x lands on t = x + s(x), dropped unless 0 <= t < cols; of several sources on one target the NEAREST wins (the smallest
 *   s * sign(D); equal shifts never share a target); a filled target is view[t] = original[winner], no interpolation;
 *   a hole (no source) copies the view of the nearest filled target on the BACKGROUND side (right when D > 0, left when D < 0), else
 *   of the nearest on the other side, else (no filled target in the row) original[t].
 *   mode RTDD_STEREO_VIEW: artistic = view.  RTDD_STEREO_ANAGLYPH: BGR (view.b, view.g, orig.r) when D >= 0 (the view is the right
 *   eye), (orig.b, orig.g, view.r) when D < 0.
 * D > 0 renders a camera moved to the right: pixels nearer than z0 move left, farther ones right.  D = 0 gives the original in both
 * modes.  The output does not depend on RTDD_OPT_FP_CONTRACT.  One kernel launch, deterministic.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size);
 * |D| > 256; a mode other than the two; a zeroParallaxDepth that is non-finite or outside [0, 255] when it is used; a zero-parallax
 * pixel outside the image when zeroX >= 0; original == artistic (not in place). */
enum rtdd_stereo_mode { RTDD_STEREO_VIEW = 0, RTDD_STEREO_ANAGLYPH = 1 };
int rtdd_simulate_stereo(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                         const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                         int rows, int cols, int disparity, float zeroParallaxDepth, int zeroX, int zeroY, int mode);

/* Relight: the depth map read as a SURFACE and lit by one light -- a directional one, or a point light anchored to the surface
 * ("light this object") that falls off with distance.  Coordinates: x right, y down, z towards the viewer; the surface is
 * z(x, y) = relief * (255 - d'), depth 0 near, 255 far as haze and stereo read it.  Every operation below is one f32 operation, rounded
 * once, NONE fused, in the order written; sqrtf and / are IEEE correctly rounded; f32 denormals are kept.
 *   d'(x, y) = fminf(fmaxf(d, 0), 255), a NaN depth is 0                    (stereo's clamp)
 *   gx = d'(min(x+1, cols-1), y) - d'(max(x-1, 0), y)     gy likewise in y  (central difference, replicated border)
 *   nx = relief * gx;  ny = relief * gy;  nz = 2                            (the unnormalised normal 2 * (-dz/dx, -dz/dy, 1))
 *   nn = ((nx*nx) + (ny*ny)) + 4
 *   DIRECTIONAL: (lx, ly, lz) = the unit vector of (x, y, z), normalised on the host in double (length sqrt(x*x + y*y + z*z)), each
 *                component rounded to f32
 *                dot = ((nx*lx) + (ny*ly)) + (2*lz)
 *                shade = fmaxf(dot, 0) / sqrtf(nn)
 *   POINT:       dA = anchorDepth when anchorX < 0, otherwise d' at (anchorX, anchorY), READ BY THE KERNEL ON THE DEVICE when it runs
 *                Lz = (relief * (255 - dA)) + z                             (the light's height in scene units)
 *                vx = light.x - (float)x;  vy = light.y - (float)y;  vz = Lz - (relief * (255 - d'))
 *                vv = ((vx*vx) + (vy*vy)) + (vz*vz)
 *                dot = ((nx*vx) + (ny*vy)) + (2*vz)
 *                shade = (fmaxf(dot, 0) / sqrtf(nn * vv)) / (1 + (vv * invR2)),  invR2 = (float)(1.0 / ((double)radius * radius)) on the
 *                host;  vv == 0: shade = 0
 *   per channel c of B, G, R:  k_c = (float)((double)diffuse * color_c / 255.0) on the host
 *                out_c = (uchar) fminf(o_c * (ambient + (k_c * shade)), 255)   (truncation, as the reference's effects)
 * Sign: the normal is (-dz/dx, -dz/dy, 1) = (relief * dd'/dx, relief * dd'/dy, 1) and the central difference is twice the derivative,
 * hence nz = 2.  A surface that gets NEARER towards the right (gx < 0) rises towards the right and faces LEFT: it is lit by a light
 * from the left and dark under one from the right.  A constant map under DIRECTIONAL (0, 0, 1), ambient 0, diffuse 1, white, gives the
 * original; relief 0 shades by distance only; diffuse 0 gives (uchar) fminf(o * ambient, 255) whatever the map.
 * The output does not depend on RTDD_OPT_FP_CONTRACT.  One kernel launch, stream-ordered, deterministic.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size); a
 * null light; an unknown kind; any non-finite float; z <= 0; a directional (x, y, z) whose length in double is zero or not finite;
 * relief outside [0, 64]; ambient or diffuse outside [0, 8]; of a POINT light (a directional light's anchor and radius need only be
 * finite: it does not use them): x or y outside [-32768, 32767], z above 65536, radius outside (0, 65536] (with these bounds nn * vv
 * stays below 2^70: no overflow, no NaN but the stated vv == 0), an anchor pixel outside the image when anchorX >= 0, an anchorDepth
 * outside [0, 255] when it is used; original == artistic (not in place). */
enum rtdd_light_kind { RTDD_LIGHT_DIRECTIONAL = 0, RTDD_LIGHT_POINT = 1 };
typedef struct rtdd_light {
    int   kind;                 /* enum rtdd_light_kind */
    float x, y, z;              /* DIRECTIONAL: the direction TOWARDS the light (any length; z > 0).
                                   POINT: (x, y) the light's position in pixels (may lie outside the image), z its height in
                                   pixels above the surface point it is anchored to (z > 0) */
    float anchorDepth;          /* POINT: the depth of that surface point when anchorX < 0 */
    int   anchorX, anchorY;     /* POINT: anchorX >= 0: the depth map's value at this pixel instead, READ BY THE KERNEL ON THE
                                   DEVICE when it runs (no host synchronisation; the call may sit behind an asynchronous estimate) */
    float radius;               /* POINT: distance in pixels at which the light has fallen to one half (> 0) */
    float relief;               /* pixels of height per unit of depth, in [0, 64]; 0: a flat surface (no shading by orientation) */
    float ambient, diffuse;     /* each in [0, 8]: gain = ambient + diffuse * colour * shade */
    uint8_t colorB, colorG, colorR;   /* the light's colour; 255, 255, 255: white */
} rtdd_light;
int rtdd_simulate_relight(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                          const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                          int rows, int cols, const rtdd_light *light /* HOST, read before the call returns */);

/* Relight with CAST SHADOWS: rtdd_simulate_relight, and in addition every pixel marches over the height field H(x, y) = relief * (255 - d'(x, y))
 * towards the light and is darkened where the surface rises above its ray.  The rules of rtdd_simulate_relight carry over: every
 * operation is one f32 operation, rounded once, NONE fused; / is IEEE correctly rounded; denormals are kept; rintf rounds half to even;
 * d', shade, k_c, Lz, vx, vy, vz and the unit vector (lx, ly, lz) are exactly rtdd_simulate_relight's.
 * The direction of the march -- it steps along the MAJOR axis of the projected direction towards the light:
 *   DIRECTIONAL: m = fmaxf(fabsf(lx), fabsf(ly));  sx = lx / m;  sy = ly / m;  rise = lz / m;  n = maxSteps      (f32, on the host;
 *                m == 0: every pixel is lit)
 *   POINT, per pixel: m = fmaxf(fabsf(vx), fabsf(vy));  m < 1: the pixel is lit;  otherwise sx = vx / m;  sy = vy / m;  rise = vz / m;
 *                n = min(maxSteps, (int)m)                        (the march ends at the light's column or row)
 * The march, for k = 1 .. n, kf = (float)k:
 *   px = x + (int)rintf(kf * sx);  py = y + (int)rintf(kf * sy);  the first k whose (px, py) lies outside the image ends the march
 *   ray = (H(x, y) + bias) + (kf * rise)
 *   occ = H(px, py) - ray
 *   q_k = 0 when !(occ > 0);  otherwise 1 when softness == 0, and fminf(occ / (kf * softness), 1) when softness > 0   (a blocker
 *         farther away gives a wider penumbra)
 *   q = max over k of q_k  (0 over no steps);  vis = 1 - (strength * q)
 * per channel c of B, G, R:  out_c = (uchar) fminf(o_c * (ambient + (k_c * (shade * vis))), 255)
 * q is a maximum of values in [0, 1]: the order of the steps does not matter.  An implementation may stop a march as soon as q == 1,
 * and for rise >= 0 as soon as ray > relief * 255 (no height reaches the ray from there on: rounding is monotonic); these are its
 * freedoms, not part of the rule.  maxSteps == 0 or strength == 0 gives rtdd_simulate_relight's bytes.  A constant map is never
 * shadowed by a light that does not stand below it (rise >= 0, so ray >= H: every directional light, a point light with Lz >= H); a
 * point light below the surface does shadow it.
 * With the stated bounds nothing produces a NaN: occ > 0 is divided by a positive kf * softness, an infinite rise gives occ = -inf.
 * The output does not depend on RTDD_OPT_FP_CONTRACT; one kernel launch, stream-ordered, deterministic, not in place.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: everything rtdd_simulate_relight refuses; a null shadow; any non-finite
 * field; any field outside the ranges below. */
typedef struct rtdd_shadow {
    int   maxSteps;    /* [0, 1024]: pixels marched towards the light along the major axis; 0: no shadows */
    float bias;        /* [0, 65536]: height (scene units = pixels) the ray starts above the surface: against self-shadowing */
    float softness;    /* [0, 65536]: 0 hard shadows; > 0: penumbra -- see q_k */
    float strength;    /* [0, 1]: the share of the diffuse term a full shadow removes */
} rtdd_shadow;
int rtdd_simulate_relight_shadowed(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                                   const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                                   int rows, int cols, const rtdd_light *light, const rtdd_shadow *shadow /* both HOST, read before the call returns */);

/* Parallax: the view of a camera that moved sideways, up or down, forward or back, rendered from the depth map (0 near, 255 far, as
 * stereo reads it) -- stereo's forward warp with a shift in x AND y that may vary over the image, so sources cross rows, the nearest
 * source wins over the whole image and holes are filled in every direction.  Every operation below is one f32 operation, rounded once,
 * NONE fused, in the order written; / is IEEE correctly rounded; rintf rounds half to even.
 *   d' = fminf(fmaxf(d, 0), 255), a NaN depth is 0, -0 counts as +0 (stereo's clamp);  z0 = zeroParallaxDepth when zeroX < 0, otherwise
 *       the depth map's value at (zeroX, zeroY), clamped alike and READ BY THE KERNEL ON THE DEVICE when it runs (no host
 *       synchronisation; the call may sit behind an asynchronous estimate)
 *   cx = (float)(cols - 1) * 0.5f;  cy = (float)(rows - 1) * 0.5f                              (the image centre, on the host)
 *   per pixel (x, y):  ax = (float)shiftX - (dolly * ((float)x - cx));  ay = (float)shiftY - (dolly * ((float)y - cy))
 *       (the shift of a point 255 depth units behind z0; with the bounds below |ax|, |ay| <= 512)
 *   SOURCE (x, y):  sx = (int)rintf((ax * (d' - z0)) / 255.0f);  sy = (int)rintf((ay * (d' - z0)) / 255.0f)     (|sx|, |sy| <= 512)
 *       it lands on the target t = (x + sx, y + sy) and is dropped when t lies outside the image
 *   WINNER:  of several sources on one target the NEAREST wins: the smallest d'; among equal d' the smallest y * cols + x.  A filled
 *       target is view[t] = original[winner], no interpolation.
 *   HOLE (a target t = (x, y) no source lands on):  ax, ay as above AT THE HOLE'S OWN POSITION;  m = fmaxf(fabsf(ax), fabsf(ay))
 *       m == 0: view[t] = original[t].  Otherwise stx = ax / m;  sty = ay / m, and the hole marches along the major axis of (ax, ay)
 *       towards the BACKGROUND side, the direction +a, the way far points move: for k = 1, 2, ...
 *           p = (x + (int)rintf((float)k * stx), y + (int)rintf((float)k * sty))
 *       the first p outside the image ends the march; the first FILLED p gives view[t] = view[p] (= original[p's winner]).  A march
 *       that ends without one is run again with both offsets negated (p = (x - (int)rintf(..), y - (int)rintf(..))); if that ends
 *       too, view[t] = original[t].
 *   artistic = view.
 * shiftX > 0 renders a camera moved to the right (stereo's D), shiftY > 0 one moved down, dolly > 0 one moved forward: points nearer
 * than z0 spread away from the image centre, farther ones move towards it.
 * Identities: shiftY == 0 and dolly == 0 gives rtdd_simulate_stereo(..., disparity = shiftX, ..., RTDD_STEREO_VIEW) byte for byte
 * (there the smallest d' IS the smallest s * sign(D), and the march is stereo's nearest filled target on the background side, then
 * on the other); shiftX == shiftY == 0 with dolly == 0, or a constant map equal to z0, gives the original.
 * The outcome never depends on the order in which sources reach a target; the output does not depend on RTDD_OPT_FP_CONTRACT.
 * Stream-ordered (a fill, a scatter and a resolve pass over 8 bytes of context-owned scratch per pixel), deterministic, not in place.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size); a
 * null view; a shift outside [-256, 256]; a dolly that is non-finite or too large (see the field); a zeroParallaxDepth that is
 * non-finite or outside [0, 255] when it is used; a zero-parallax pixel outside the image when zeroX >= 0; original == artistic.
 * RTDD_ERR_NOMEM, before any launch, when the scratch cannot be allocated. */
typedef struct rtdd_parallax {
    int   shiftX, shiftY;       /* each in [-256, 256]: the shift in pixels of a point 255 depth units behind the zero-parallax depth;
                                   shiftX > 0: the camera moved to the right (stereo's D), shiftY > 0: the camera moved down */
    float dolly;                /* > 0: the camera moved forward (near points spread away from the image centre), < 0: back.  Finite,
                                   |dolly| * max(cols - 1, rows - 1) / 2 <= 256 evaluated in double */
    float zeroParallaxDepth;    /* used when zeroX < 0: finite, in [0, 255] */
    int   zeroX, zeroY;         /* zeroX >= 0: the depth map's value at this pixel instead, READ BY THE KERNEL ON THE DEVICE when it runs */
} rtdd_parallax;
int rtdd_simulate_parallax(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                           const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                           int rows, int cols, const rtdd_parallax *view /* HOST, read before the call returns */);

/* Parallax over TWO LAYERS: rtdd_simulate_parallax with a BACKGROUND PLATE -- the scene without the object, colour and depth, as
 * rtdd_remove_object writes it -- that fills what the camera's move uncovers, instead of a smear of the background's edge pixel; and
 * with the view's own depth map and a coverage map as outputs, so that artistic / depthOut are original / depth of every other call.
 * Everything not named here is rtdd_simulate_parallax's, bit for bit: d', z0, (ax, ay), the source shift, the march, every f32
 * operation rounded once with nothing fused.
 *   SOURCES:  every pixel of the front layer (original, depth), as there.  With a plate, every pixel of the plate too: d' of plateDepth,
 *       the colour of plate, the same (ax, ay) at its own position.  z0 is the same for both layers; in the pixel form it is read from
 *       the FRONT map at (zeroX, zeroY), on the device, when the kernel runs.
 *   WINNER:  the smallest d'; among equal d' the FRONT layer; among equal d' and layer the smallest y * cols + x.
 *       A plate pixel whose d' equals the front's d' at the SAME pixel lands on the same target with the same depth: it always loses, and
 *       an implementation may skip it without reading its colour (a plate from rtdd_remove_object then costs work on its hole alone).
 *   CRACK:  a slanted surface is stretched by the warp and one-pixel gaps open between its own sources, where the plate would shine
 *       through.  Take a BACK-won target t, with (ax, ay), m, stx, sty at t as the hole rule forms them, and m != 0:
 *           p+ = t + ((int)rintf(stx), (int)rintf(sty)),  p- = t - ((int)rintf(stx), (int)rintf(sty))        (the march's step k = 1)
 *       t is a crack iff p+ and p- are both inside the image, both FRONT-won, and both winners' d' are STRICTLY smaller than the d' of
 *       t's winner.  A crack takes the source of p+.  A crack's neighbours are front-won, so they are never cracks: no recursion.  A
 *       one-pixel gap between an object and front-layer background at the plate's own depth is a true disocclusion (equal d'): it keeps
 *       the plate's pixel.  A surface stretched by more than 2 x opens gaps two pixels wide, which this rule does not close.
 *   HOLE (a target neither layer lands on):  the march as there, over "filled" = a source of either layer landed.  The hole takes the
 *       SOURCE of the first filled p: p's winner, or, where p is a crack, the crack's source.
 *   OUTPUTS:  artistic[t] = the colour of t's source, from original or plate by its layer.  depthOut[t] = that source's d' (the clamped
 *       value with -0 folded into +0, never the map's raw bits).  A hole that both marches leave, or one with m == 0, gets original[t]
 *       and the front d'(t).  coverage[t] = 0 front-won, 1 back-won, 2 a crack, 3 a hole filled by a march, 4 a hole left as the original.
 *       The codes are chosen so that rtdd_remove_object(artistic, depthOut, coverage, ..., select = 3) fills the remaining smears by
 *       push-pull.
 * Identities: with plate == NULL artistic is rtdd_simulate_parallax's byte for byte; so it is with a plate equal to the front layer (the
 * same arrays, or copies), and with a plate whose DEPTH has the front's d' everywhere, whatever its colours; shiftX == shiftY == 0 with
 * dolly == 0 gives original, the front d' and coverage 0 everywhere, with no plate or a plate that is nowhere NEARER than the front
 * layer at the same pixel (every background plate; a plate pixel that is nearer wins its own target by the WINNER rule, motion or
 * none).  The outcome never depends on the order in which sources reach a
 * target, nor on RTDD_OPT_FP_CONTRACT.  Stream-ordered, the same scratch and passes as rtdd_simulate_parallax; with plate, depthOut and
 * coverage all NULL the launches are that call's.  Not in place: a healed time-out runs the call again, and the second run must read
 * what the first one read.  RTDD_VERSION is unchanged: a host finds the symbol by name.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: everything rtdd_simulate_parallax refuses of the images and the view;
 * exactly one of plate / plateDepth null; platePitch < 3 * cols; plateDepthPitch or depthOutPitch below 4 * cols, or either image
 * misaligned as depth's rule says; coveragePitch < cols; artistic equal to original or plate; depthOut equal to depth or plateDepth. */
int rtdd_simulate_parallax_layered(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                                   const float *depth, size_t depthPitch,                 /* the FRONT layer */
                                   const uint8_t *plate, size_t platePitch,
                                   const float *plateDepth, size_t plateDepthPitch,       /* the BACK layer: both or neither NULL */
                                   uint8_t *artistic, size_t artisticPitch,
                                   float *depthOut, size_t depthOutPitch,                 /* may be NULL: no depth is written */
                                   uint8_t *coverage, size_t coveragePitch,               /* may be NULL: u8, rows x cols */
                                   int rows, int cols, const rtdd_parallax *view /* HOST, read before the call returns */);

/* Ambient occlusion: the third term of relight's lighting model.  The height field H(x, y) = relief * (255 - d'(x, y)) of
 * rtdd_simulate_relight_shadowed is searched, from every pixel, along 4 or 8 fixed compass directions over `radius` pixels for its
 * HORIZON; a pixel whose horizons stand high -- a crease, the foot of an object against a wall, the inside of a fold -- loses its
 * ambient light.  Alone it darkens the original or renders the occlusion as a gray map; under a light it is rtdd_simulate_relight
 * with the ambient term occluded.  The rules of rtdd_simulate_relight carry over: every operation is one f32 operation, rounded once,
 * NONE fused, in the order written; sqrtf and / are IEEE correctly rounded; denormals are kept; d', shade, k_c and every quantity of
 * the light are exactly rtdd_simulate_relight's.
 *   H(x, y) = relief * (255 - d'(x, y))          relief: ao.relief when light == NULL, light->relief otherwise (the two must agree)
 *   directions j = 0 .. 7:  (ux, uy) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1);  directions == 4 uses j = 0, 2, 4, 6 only
 *   inv_j[k], k = 1 .. radius, on the host in double, rounded to f32 once:
 *       axis directions (j even):  (float)(1.0 / (double)k)
 *       diagonals       (j odd):   (float)(1.0 / ((double)k * sqrt(2.0)))
 *   per pixel and direction, for k = 1 .. radius:
 *       p = (x + k*ux, y + k*uy);  the first p outside the image ends this direction's march
 *       rise = (H(p) - H(x, y)) - bias
 *       t_k  = rise * inv_j[k]                                   (the tangent of the elevation of p seen from the pixel)
 *   tmax_j = max(0, max over k of t_k)                           (a horizon below the pixel's own plane counts as 0)
 *   occ_j  = tmax_j / sqrtf(1 + (tmax_j * tmax_j))               (the sine of the horizon angle)
 *   s    = the occ_j added in ascending j, left to right: ((occ_0 + occ_1) + occ_2) + ...   (4 directions: ((occ_0 + occ_2) + occ_4) + occ_6)
 *   mean = s * (1 / directions)                                  (0.25f or 0.125f: exact)
 *   ao   = 1 - (strength * mean)                                 (in [0, 1] up to the last rounding; the bytes below truncate towards zero)
 * per channel c of B, G, R:
 *   RTDD_AO_SHADE, light == NULL:  out_c = (uchar)(o_c * ao)
 *   RTDD_AO_SHADE, light != NULL:  out_c = (uchar) fminf(o_c * ((ambient * ao) + (k_c * shade)), 255)     (relight, its ambient term occluded)
 *   RTDD_AO_MAP:                   out_B = out_G = out_R = (uchar)(255 * ao);  `original` is validated but not read; light must be NULL
 * The maximum over k does not depend on the order of the steps.  No height exceeds relief * 255 and rounding is monotonic, so once
 * ((relief * 255 - H(x, y)) - bias) * inv_j[k] <= tmax_j no later step can win: an implementation may stop a direction there, and it may
 * treat positions outside the image as a height of minus infinity.  Both are its freedoms, not part of the rule.
 * Identities: radius == 0, strength == 0, relief == 0 or a constant map give the original (light == NULL) or rtdd_simulate_relight's
 * bytes (light != NULL); RTDD_AO_MAP gives 255 everywhere in those cases.  Nothing produces a NaN: rise is finite and inv_j[k] is
 * finite and positive.
 * The output does not depend on RTDD_OPT_FP_CONTRACT; one kernel launch, stream-ordered, deterministic, not in place.  A point light's
 * anchor pixel is read by the kernel on the device, as in rtdd_simulate_relight.  Cast shadows are not combined with it here:
 * rtdd_simulate_lighting renders both.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size); a
 * null ao; an unknown mode; directions other than 4 or 8; any non-finite field; any field outside the ranges below; RTDD_AO_MAP with a
 * light; with a light, everything rtdd_simulate_relight refuses of it, and ao->relief != light->relief; original == artistic. */
enum rtdd_ao_mode { RTDD_AO_SHADE = 0, RTDD_AO_MAP = 1 };
typedef struct rtdd_ambient_occlusion {
    int   mode;        /* enum rtdd_ao_mode */
    int   directions;  /* 4 or 8 */
    int   radius;      /* [0, 64]: pixels marched in every direction; 0: no occlusion */
    float relief;      /* [0, 64]: used when light == NULL; otherwise it must equal light->relief bit for bit */
    float bias;        /* [0, 65536]: height the horizon must clear before it counts: against noise in the map */
    float strength;    /* [0, 1] */
} rtdd_ambient_occlusion;
int rtdd_simulate_ambient_occlusion(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                                    const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                                    int rows, int cols, const rtdd_ambient_occlusion *ao,
                                    const rtdd_light *light /* may be NULL */);   /* both HOST, read before the call returns */

/* Lighting: the WHOLE lighting model in one call -- rtdd_simulate_relight's diffuse shade, rtdd_simulate_relight_shadowed's cast
 * shadow on it and rtdd_simulate_ambient_occlusion's occlusion of the ambient term: an object that throws a shadow AND sits in a
 * darkened crease where it meets the ground.  Every call ends in a truncated, clamped uchar, so two calls cannot be composed
 * afterwards; this one renders the three terms per pixel.  Nothing here is new arithmetic -- every operation is one f32 operation,
 * rounded once, NONE fused, in the order written; sqrtf and / are IEEE correctly rounded; denormals are kept:
 *   d', shade, k_c, Lz and every quantity of the light:       exactly rtdd_simulate_relight's
 *   H(x, y) = relief * (255 - d'(x, y)),  relief = light->relief = ao->relief (the two must agree bit for bit)
 *   m, sx, sy, rise, n, the march for k = 1 .. n (px, py, ray, occ, q_k), q;  vis = 1 - (shadow->strength * q):
 *                                                             exactly rtdd_simulate_relight_shadowed's, march included
 *   inv_j[k], the marches p, rise, t_k, tmax_j, occ_j, s in ascending j, mean;  ao = 1 - (ao->strength * mean):
 *                                                             exactly rtdd_simulate_ambient_occlusion's
 * per channel c of B, G, R:
 *   out_c = (uchar) fminf(o_c * ((ambient * ao) + (k_c * (shade * vis))), 255)          (truncation, as every effect)
 * The freedoms of the two marches (their early exits, minus infinity outside the image) carry over; they are not part of the rule.
 * Identities, byte for byte (vis is then exactly 1, ao exactly 1):
 *   shadow->maxSteps == 0 or shadow->strength == 0:  rtdd_simulate_ambient_occlusion(..., ao, light)'s bytes
 *   ao->radius == 0 or ao->strength == 0:            rtdd_simulate_relight_shadowed's bytes
 *   both together:                                   rtdd_simulate_relight's bytes
 * Nothing produces a NaN (see the two calls).  The output does not depend on RTDD_OPT_FP_CONTRACT; one kernel launch (a disabled term
 * costs nothing: the launch is then the kernel of what is left), stream-ordered, deterministic, not in place.  A point light's anchor
 * pixel is read by the kernel on the device, as in rtdd_simulate_relight.  RTDD_VERSION is unchanged: a host finds the symbol by name.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: everything rtdd_simulate_relight_shadowed refuses of the images, the light
 * and the shadow; everything rtdd_simulate_ambient_occlusion refuses of ao under a light, ao->relief != light->relief included; a null
 * light, shadow or ao; ao->mode other than RTDD_AO_SHADE; original == artistic. */
int rtdd_simulate_lighting(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                           const float *depth, size_t depthPitch, uint8_t *artistic, size_t artisticPitch,
                           int rows, int cols, const rtdd_light *light, const rtdd_shadow *shadow,
                           const rtdd_ambient_occlusion *ao /* all three HOST, read before the call returns */);

/* Composite a layer: a SPRITE (u8 x 4: B, G, R, A; straight alpha) is inserted into the photograph at a depth, and the scene's own depth
 * map hides the parts of it that lie behind nearer things -- a title behind the subject, an object on the floor, a logo on the far wall.
 * The call also writes the composite's depth map (the layer's depth where the layer won, the scene's elsewhere), so that every effect
 * above treats the inserted object as part of the scene: artistic and depthOut of this call are original and depth of the next one,
 * another layer included (one layer per call).  Depth 0 is near, 255 far, as every effect reads it.  Integers are exact; every f32
 * operation below is one operation, rounded once, NONE fused; / on floats is IEEE correctly rounded.  Per image pixel (px, py):
 *   1. SPRITE COORDINATE in 1/256 texel, floor division in 64 bits:
 *        U = floor(((2 (px - x) + 1) * 32768) / scale) - 128          V likewise from py, y
 *      (the pixel's centre, in texels the texel centres at the integers).  The pixel is COVERED iff 0 <= U + 128 < 256 * layer.cols and
 *      0 <= V + 128 < 256 * layer.rows.  An uncovered pixel gets artistic = original and depthOut = depth: the depth's bits are copied,
 *      a NaN included.
 *   2. SAMPLE (c_B, c_G, c_R, a):
 *      RTDD_LAYER_NEAREST:  the texel (floor((U + 128) / 256), floor((V + 128) / 256)) as it is.
 *      RTDD_LAYER_BILINEAR: iu = floor(U / 256), fu = U - 256 iu, likewise iv, fv; the four taps (iu | iu + 1, iv | iv + 1), each index
 *        clamped into the sprite; tap weights w = (256 - fu | fu) * (256 - fv | fv), which sum to 65536.  The interpolation is
 *        ALPHA-WEIGHTED, so a transparent texel's colour never bleeds:  A = sum of w a,  C_c = sum of w a c  (A < 2^24, C_c < 2^32);
 *        a = (A + 32768) >> 16;  c = A ? (C_c + (A >> 1)) div A : 0.
 *   3. LAYER DEPTH, a plane: dd = (x1-x0)^2 + (y1-y0)^2;  n = (px-x0)(x1-x0) + (py-y0)(y1-y0) clamped to [0, dd] (then n < 2^31);
 *        z = dd ? depth0 + ((depth1 - depth0) * ((float)n / (float)dd)) : depth0
 *   4. VISIBILITY v in 0 .. 256:  d' = fminf(fmaxf(d, 0), 255), a NaN depth is 0 (stereo's clamp);  diff = d' - z
 *        feather == 0:  v = diff >= 0 ? 256 : 0                       (at equal depth the layer is in front)
 *        otherwise:     t = (diff / feather) + 0.5f;  v = (int)(fminf(fmaxf(t, 0), 1) * 256.0f)
 *   5. BLEND, exact in 32 bits unsigned:  e = a * opacity * v  (<= E = 255 * 255 * 256 = 16646400);
 *        per channel c of B, G, R:  out_c = (c_c * e + o_c * (E - e) + E / 2) div E
 *   6. DEPTH OUT:  depthOut = (2 e >= E) ? z : d                       (d itself, not d': bits copied)
 * Identities: opacity 0, a sprite of alpha 0, or a layer behind everything (depth 255, feather 0, every d < 255) give the original and
 * a bit copy of the depth; RTDD_LAYER_BILINEAR at scale 256 is RTDD_LAYER_NEAREST (fu = fv = 0); an opaque sprite at depth 0 with
 * feather 0 and opacity 255 is a paste.  No mip-mapping: a sprite minified below roughly 1/2 (scale < 128) aliases.  A sprite that lands
 * wholly outside the image is not an error: the call then copies.
 * One kernel launch that stores every pixel of artistic, and of depthOut when given, exactly once; asynchronous, stream-ordered,
 * deterministic; the output does not depend on RTDD_OPT_FP_CONTRACT.  Not in place: a healed time-out runs the call again, and the second
 * run must read what the first one read.  RTDD_VERSION is unchanged: a host finds the symbol by name.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: the rules of the three effects (null pointers, pitches, image size; the
 * f32 alignment rule for depthOut too, and depthOutPitch >= 4 * cols); original == artistic; depth == depthOut; a null layer; a null
 * sprite, or spritePitch < 4 * layer.cols; any field outside the ranges below; an unknown filter; a non-finite float. */
enum rtdd_layer_filter { RTDD_LAYER_NEAREST = 0, RTDD_LAYER_BILINEAR = 1 };
typedef struct rtdd_layer {
    int   rows, cols;           /* the sprite's size in texels, 1 .. 16384 each */
    int   x, y;                 /* where the sprite's top-left corner lands in the image, each in [-16384, 16383]; may lie outside */
    int   scale;                /* size on screen in 1/256: 256 = texel for pixel; 16 .. 4096 */
    int   filter;               /* enum rtdd_layer_filter */
    int   opacity;              /* 0 .. 255 */
    int   x0, y0, x1, y1;       /* the layer's depth is a plane: depth0 at (x0, y0), depth1 at (x1, y1); image coordinates, each in
                                   [-16384, 16383]; (x0, y0) == (x1, y1): the constant depth0 */
    float depth0, depth1;       /* finite, in [0, 255] */
    float feather;              /* finite, >= 0: the depth interval over which the scene takes over from the layer; 0: a hard edge */
} rtdd_layer;                   /* 56 bytes, ints and floats only */
int rtdd_composite_layer(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                         const float *depth, size_t depthPitch,
                         const uint8_t *sprite, size_t spritePitch,     /* DEVICE, u8 x 4 */
                         uint8_t *artistic, size_t artisticPitch,
                         float *depthOut, size_t depthOutPitch,         /* may be NULL: no depth is written */
                         int rows, int cols, const rtdd_layer *layer /* HOST, read before the call returns */);

/* Remove an object, and lift it out as a sprite: the opposite of rtdd_composite_layer.  A MASK (u8, rows x cols, DEVICE) says which
 * pixels are the object -- what the wand, the lasso or a region code (RTDD_IMG_REGION_CODE) selected.  rtdd_lift_layer cuts the selection
 * out as a sprite for rtdd_composite_layer; rtdd_remove_object fills what it leaves behind, colour AND depth, by a push-pull over a
 * pyramid, and hands on the depth map like rtdd_composite_layer: insert, delete, move.  Depth 0 is near, 255 far.
 *   d' = d > 0 ? fminf(d, 255) : +0        (= fminf(fmaxf(d, 0), 255) with the zero's sign settled: a NaN, -0 and every negative depth are +0)
 * Integers are exact; every f32 operation below is one operation, rounded once, NONE fused; / is IEEE correctly rounded.
 *   CLASSES at level 0.  A pixel is SELECTED iff its mask byte != 0 (select == 0) or == select (select 1..255: a region code), and
 *     ELIGIBLE iff d' >= sourceMinDepth.
 *       HOLE:      selected, or eligible and within Chebyshev distance `grow` of a selected pixel of the image (the ring never eats into a
 *                  nearer neighbour)
 *       SOURCE:    not a hole, and eligible
 *       BYSTANDER: everything else: kept, and never read as a source
 *   LEVELS.  Level 0 is rows x cols, level k+1 is ceil(r / 2) x ceil(c / 2); the chain ends at the first level that is 1 x 1.  A sample is
 *     (B, G, R) in 0..255, a depth in f32 and a valid bit.  At level 0 the valid samples are the sources, with depth d'.
 *   PULL.  Sample (i, j) of level k+1 from its children (2i+a, 2j+b) that exist and are valid, in the order (0,0), (0,1), (1,0), (1,1);
 *     n their count.  n == 0: not valid.  Otherwise per channel  c = (2 * sum c + n) div (2 n),  and the depth
 *     (((d1 + d2) + d3) + d4) / (float)n  over the valid children in that order.
 *   PUSH, from the level below the top down to level 0.  A sample (y, x) of level k that is not valid (at level 0: a hole; bystanders
 *     are left alone) is filled from level k+1:  yn = y >> 1;  yf = (y & 1) ? yn + 1 : yn - 1, clamped into the coarse level; x likewise.
 *       per channel  c = (9 c[yn,xn] + 3 c[yn,xf] + 3 c[yf,xn] + c[yf,xf] + 8) >> 4
 *       depth        t = 9 * d[yn,xn];  t = t + 3 * d[yn,xf];  t = t + 3 * d[yf,xn];  t = t + d[yf,xf];  depth = t * 0.0625f
 *     (each product and each sum rounded on its own).  The filled sample is valid iff [yn,xn] is: with the chain run to 1 x 1 a coarse
 *     level is wholly valid or, if the image has no source at all, wholly invalid.
 *   OUTPUT.  A filled hole pixel gets the colour and the depth it was filled with.  Every other pixel gets original's bytes and depth's
 *     bits, a NaN included -- the hole pixels of an image without a single source too.
 * Identities: no selected pixel, and no source anywhere, each give a bit copy of both inputs; a hole whose sources all have one colour
 * is filled with exactly that colour ((16 c + 8) >> 4 = c; the depth may differ by a rounding).
 *   LIFT.  Texel (u, v) of the sprite is image pixel (x + u, y + v): inside the image and selected (by mask and select alone: no grow,
 *     no depth) it is (B, G, R, 255) from original, otherwise (0, 0, 0, 0).  Every texel of the sprite is stored exactly once.
 * The three calls together: with a sprite box that covers the selection, grow = 0 and any sourceMinDepth, rtdd_composite_layer of the
 * lifted sprite onto rtdd_remove_object's two outputs (layer.rows / cols the sprite's, x, y the lift's, scale 256, RTDD_LAYER_NEAREST,
 * opacity 255, depth0 = 0 with (x0, y0) == (x1, y1), feather 0) gives `original` back byte for byte.
 * Both calls: asynchronous, stream-ordered, deterministic, independent of RTDD_OPT_FP_CONTRACT; not in place (a healed time-out runs
 * the call again, and the second run must read what the first one read).  rtdd_remove_object stores every pixel of artistic, and of
 * depthOut when given, exactly once; it keeps its coarse levels in the context's table buffer.  RTDD_VERSION is unchanged.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: rtdd_composite_layer's image rules for every pointer, with maskPitch >=
 * cols and spritePitch >= 4 * spriteCols; original == artistic; depth == depthOut; a null mask; a null removal; any field outside its
 * range; a non-finite float. */
typedef struct rtdd_removal {
    int   select;               /* 0: a pixel is selected iff its mask byte != 0;  1 .. 255: iff its mask byte == select (a region code) */
    int   grow;                 /* 0 .. 8: the hole also takes the eligible pixels within this Chebyshev distance of a selected pixel */
    float sourceMinDepth;       /* finite, in [0, 255]: only pixels at least this far are sources of the fill; 0: every pixel */
} rtdd_removal;                 /* 12 bytes */
int rtdd_remove_object(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                       const float *depth, size_t depthPitch,
                       const uint8_t *mask, size_t maskPitch,           /* DEVICE, u8, rows x cols */
                       uint8_t *artistic, size_t artisticPitch,
                       float *depthOut, size_t depthOutPitch,           /* may be NULL: no depth is written */
                       int rows, int cols, const rtdd_removal *removal /* HOST, read before the call returns */);
int rtdd_lift_layer(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                    const uint8_t *mask, size_t maskPitch,              /* DEVICE, u8, rows x cols */
                    int rows, int cols, int select /* 0 .. 255, as rtdd_removal.select */,
                    int x, int y,                                       /* the sprite's corner in the image, each in [-16384, 16383] */
                    uint8_t *sprite, size_t spritePitch,                /* DEVICE, u8 x 4, written */
                    int spriteRows, int spriteCols                      /* 1 .. 16384 each */);

/* Refine a mask: the exact Euclidean distance transform of a selection, and the four things it is wanted for -- grow, shrink, outline and
 * feather -- between the selecting calls (the wands, the lasso, rtdd_segment_surfaces) and the calls that use a selection
 * (rtdd_remove_object, rtdd_lift_layer, a plate).  A MASK is u8, rows x cols, on the DEVICE.  Everything is exact in 32-bit integers
 * (rows^2 + cols^2 < 2^31, rtdd_lift_layer's image rule); E is a minimum of integers, so the result cannot depend on the schedule.
 *   SELECTED: rtdd_removal.select's rule -- select == 0: the mask byte != 0;  select 1..255: the mask byte == select.
 *   E(p), for a pixel p = (px, py): the minimum over the image's pixels q of the OTHER class (the unselected ones for a selected p, the
 *     selected ones for an unselected p) of (px - qx)^2 + (py - qy)^2.  No pixels exist outside the image: an object that touches the
 *     border has no boundary there.  E >= 1 whenever it exists; where the other class is empty E is infinite.
 * rtdd_mask_distance, reach in 1..1024:
 *     dist2(p) = -E if p is selected, +E if not, wherever E <= reach * reach;  -RTDD_DISTANCE_FAR or +RTDD_DISTANCE_FAR otherwise.
 *   It is never 0.  The cut-off is the Euclidean one: around a single selected pixel the finite values are exactly the disc
 *   dx^2 + dy^2 <= reach^2, and the corners of its (2 reach + 1)^2 box are FAR.  Every pixel of dist2 is stored exactly once.  dist2
 *   follows the f32 image alignment rule (pointer and pitch multiples of 4), dist2Pitch >= 4 * cols.
 * rtdd_refine_mask writes one byte per pixel, by refine->op:
 *   RTDD_REFINE_GROW:     out = (selected || E <= outer2) ? 255 : 0                     outer2 in 1..1024^2 (inner2 is not read)
 *   RTDD_REFINE_SHRINK:   out = (selected && E > inner2) ? 255 : 0                      inner2 in 1..1024^2 (outer2 is not read)
 *   RTDD_REFINE_OUTLINE:  out = ((selected && E <= inner2) || (!selected && E <= outer2)) ? 255 : 0
 *                         inner2, outer2 each in 0..1024^2 and not both 0; 0: that side of the outline is empty
 *   RTDD_REFINE_FEATHER:  lo < hi, both finite, in [-1023.5, 1023.5].  Every f32 operation is one operation, rounded once, NONE fused;
 *                         sqrtf and / are IEEE correctly rounded:
 *       t = sqrtf((float)E)                              (E <= 2^20 whenever it matters: the conversion is exact)
 *       s = selected ? 0.5f - t : t - 0.5f               (the boundary runs midway between pixel centres: s <= -0.5 inside, >= 0.5 outside)
 *       u = (hi - s) / (hi - lo);  u = fminf(fmaxf(u, 0), 1);  out = (int)(u * 255.0f + 0.5f)
 *                         E infinite: 255 if selected, 0 if not.  lo = -w, hi = 0 is an inner feather of w pixels that never reaches
 *                         beyond the selection; lo = -w / 2, hi = w / 2 straddles the boundary.
 *   (lo, hi are not read by the first three, inner2 and outer2 not by the feather.)  The reach is derived on the host and never shown:
 *   the smallest R with R^2 >= max(inner2, outer2), or for the feather the smallest integer R >= max(|lo|, |hi|) + 0.5; R <= 1024 by the
 *   ranges above.  With that R a pixel whose E lies beyond the reach saturates to the byte the rule gives it with its true E -- for the
 *   thresholds because E > R^2 >= the threshold; for the feather because rounding is monotone: t >= R gives s <= 0.5 - R <= lo inside
 *   (u >= 1) and s >= R - 0.5 >= hi outside (u <= 0), in f32 as in the reals.  So THE OUTPUT IS THE RULE APPLIED TO THE UNBOUNDED E.
 *   The distance map is never stored for this call.
 * rtdd_lift_layer_matte is rtdd_lift_layer with an ALPHA image (u8, rows x cols, e.g. a feathered mask) in place of mask and select:
 *   texel (u, v) is (B, G, R, a), a the alpha byte of image pixel (x + u, y + v); (0, 0, 0, 0) where a == 0 or the pixel lies outside the
 *   image.  With an alpha of only 0 and 255 it writes rtdd_lift_layer(select = 0)'s bytes.  For ANY alpha, rtdd_composite_layer of the
 *   sprite onto `original` itself (scale 256, RTDD_LAYER_NEAREST, opacity 255, depth0 = 0 with (x0, y0) == (x1, y1), feather 0) gives
 *   `original` byte for byte: (o e + o (E - e) + E / 2) div E = o.  A soft edge carries the colour it had, not a halo.
 * All three: asynchronous, stream-ordered, deterministic, independent of RTDD_OPT_FP_CONTRACT; not in place (a healed time-out runs the
 * call again, and the second run must read what the first one read).  The first two keep their column pass in the context's table
 * buffer.  RTDD_VERSION is unchanged: a host finds the symbols by name.
 * Refused on the host (RTDD_ERR_INVALID), before any launch: rtdd_lift_layer's image rules (null pointers, negative sizes, the image
 * size, maskPitch, outPitch, alphaPitch >= cols, dist2Pitch >= 4 * cols, the f32 alignment rule for dist2, the sprite's rules);
 * out == mask; dist2 == mask; sprite == original; select outside [0, 255]; reach outside [1, 1024]; a null refine; an unknown op; any
 * field the op reads outside its range; lo >= hi; a non-finite lo or hi. */
#define RTDD_DISTANCE_FAR 0x7fffffff
enum rtdd_refine_op { RTDD_REFINE_GROW = 0, RTDD_REFINE_SHRINK = 1, RTDD_REFINE_OUTLINE = 2, RTDD_REFINE_FEATHER = 3 };
typedef struct rtdd_mask_refine {
    int   select;               /* 0: a pixel is selected iff its mask byte != 0;  1 .. 255: iff its mask byte == select (a region code) */
    int   op;                   /* enum rtdd_refine_op */
    int   inner2, outer2;       /* squared distances: how far the rule reaches into the selection, and out of it */
    float lo, hi;               /* the feather's ramp, in pixels from the boundary (negative: inside): 255 at s <= lo, 0 at s >= hi */
} rtdd_mask_refine;             /* 24 bytes, ints and floats only */
int rtdd_mask_distance(rtdd_ctx *ctx, const uint8_t *mask, size_t maskPitch,        /* DEVICE, u8, rows x cols */
                       int rows, int cols, int select /* 0 .. 255 */, int reach /* 1 .. 1024 */,
                       int32_t *dist2, size_t dist2Pitch                            /* DEVICE, i32, rows x cols, written */);
int rtdd_refine_mask(rtdd_ctx *ctx, const uint8_t *mask, size_t maskPitch,          /* DEVICE, u8, rows x cols */
                     int rows, int cols, const rtdd_mask_refine *refine /* HOST, read before the call returns */,
                     uint8_t *out, size_t outPitch                                  /* DEVICE, u8, rows x cols, written */);
int rtdd_lift_layer_matte(rtdd_ctx *ctx, const uint8_t *original, size_t originalPitch,
                          const uint8_t *alpha, size_t alphaPitch,                  /* DEVICE, u8, rows x cols */
                          int rows, int cols,
                          int x, int y,                                             /* the sprite's corner in the image, each in [-16384, 16383] */
                          uint8_t *sprite, size_t spritePitch,                      /* DEVICE, u8 x 4, written */
                          int spriteRows, int spriteCols                            /* 1 .. 16384 each */);

/* ---- whole-estimate driver ------------------------------------------------
 * One depth estimate = the loop body of src/main.cpp:232-295, run as a single stream-ordered launch
 * sequence with the gray pyramid, f32 pyrUp and u8 conversion ON THE DEVICE (the reference round-trips
 * through the host for cv::pyrDown / cv::pyrUp).  The context owns the pyramid images, like main.cpp
 * owns its GpuMats (src/main.cpp:117-137).  The OpenCV ops are third party: the formulas used are
 * stated in oracle/rtdd_cascade_oracle.c. */
enum rtdd_pyramid_image_kind {
    RTDD_IMG_ORIGINAL = 0,          /* u8x3, level 0 only */
    RTDD_IMG_GRAY = 1,              /* u8, ceil-sized chain (cv::pyrDown's default size) */
    RTDD_IMG_SCRIBBLE = 2,          /* u8, 255 = Dirichlet */
    RTDD_IMG_EDITED = 3,            /* u8x3 */
    RTDD_IMG_DEPTH = 4,             /* f32 */
    RTDD_IMG_DEPTH_U8 = 5,          /* u8, level 0 only */
    RTDD_IMG_ARTISTIC = 6,          /* u8x3, level 0 only: output of the effect calls */
    RTDD_IMG_GUIDE_BGR = 7,         /* u8x3 on every level, ceil-sized chain like RTDD_IMG_GRAY; level 0 IS RTDD_IMG_ORIGINAL.  The levels above 0:
                                       RTDD_ERR_STATE until a call of rtdd_pyramid_set_guide with RTDD_GUIDE_BGR has made them */
    /* the depth regions (rtdd_pyramid_set_regions): RTDD_ERR_STATE until its first call with non-zero flags has made them */
    RTDD_IMG_REGION_EDITED = 8,     /* u8x3, level 0 only: what a paint call is given as `edited` to paint a region (the label is the region id) */
    RTDD_IMG_REGION_MASK = 9,       /* u8, level 0 only: ... and as `scribble` */
    RTDD_IMG_REGION_CODE = 10       /* u8 on every level, sized like RTDD_IMG_SCRIBBLE: the codes the level's solve reads */
};
int rtdd_pyramid_levels(int rows, int cols);             /* src/main.cpp:95 */
int rtdd_pyramid_create(rtdd_ctx *ctx, int rows, int cols);   /* main.cpp:92-155 minus I/O: images, depth := 255, rtdd_allocate */
int rtdd_pyramid_destroy(rtdd_ctx *ctx);
/* Batched estimates (BASELINE configs[3]: independent images, several per GPU).  The coarse levels of one image occupy a fraction of the
 * chip -- 120 x 67 and 240 x 135 are 0.7 of a 1080p estimate's time on ~135 of 512 workgroup slots -- so `images` pyramids of ONE size on one
 * context run every level of all images in the same launches (blockIdx.z = image): rtdd_estimate_depth_batch.  rtdd_pyramid_select
 * says which image rtdd_pyramid_set_image / _set_annotation / _image (and rtdd_download of what it returns), rtdd_estimate_depth and
 * rtdd_refine_depth address (0 after creation).  Every image's maps are bit for bit those of a single-image pyramid.  Live frames
 * (rtdd_live_submit) need a single-image pyramid. */
int rtdd_pyramid_create_batch(rtdd_ctx *ctx, int rows, int cols, int images);
int rtdd_pyramid_select(rtdd_ctx *ctx, int index);
int rtdd_pyramid_batch(rtdd_ctx *ctx);                   /* the number of images of the context's pyramid (0: none) */
int rtdd_estimate_depth_batch(rtdd_ctx *ctx, int maxIterations);   /* rtdd_estimate_depth for every image of the batch; asynchronous */
/* What the most recent estimate ran on pyramid level `level` (0 = finest): the rtdd_solve_info of that level's solve, and how many images
 * each of its sweep launches covered (a batch: all of them in the same launches, or 1 = image after image, each with the launch a single
 * solve gets).  The choice is a function of the level's size AND of the batch size, so that a log line / a test can name the kernel
 * configuration a timed batch actually ran (tests/test_gpu_batch.py pins the ones bench.py times).  info->temporal_depth is the NOMINAL
 * number of sweeps per launch / exchange here (rtdd_last_solve_info reports the last launch's, which may be the short tail block; a level
 * that is one tile runs all its sweeps in one launch).  imagesPerLaunch may be NULL. */
int rtdd_pyramid_level_info(rtdd_ctx *ctx, int level, rtdd_solve_info *info, int *imagesPerLaunch);
/* image: DEVICE pointer to an interleaved BGR u8 image; builds the gray pyramid, edited[0] := image, scribble[0] := 0 */
int rtdd_pyramid_set_image(rtdd_ctx *ctx, const uint8_t *bgr, size_t pitch);
/* The guide of the pyramid's estimates (enum rtdd_guide above; RTDD_GUIDE_GRAY after rtdd_pyramid_create / _create_batch: the reference's
 * behaviour).  With RTDD_GUIDE_BGR every per-level solve of rtdd_estimate_depth, rtdd_estimate_depth_batch, rtdd_live_submit / _ex and
 * rtdd_refine_depth takes level l of a COLOUR pyramid instead of RTDD_IMG_GRAY: level 0 is the original image, level l is cv::pyrDown of
 * level l - 1 per channel (OpenCV filters channels independently) -- the arithmetic and the ceil-sized chain of rtdd_pyrdown_gray, channel by
 * channel (RTDD_IMG_GUIDE_BGR).  The first request for BGR allocates the coarse colour levels (RTDD_ERR_NOMEM before anything is launched)
 * and, if an image has been set, builds them for every image of a batch; while the guide is BGR rtdd_pyramid_set_image builds the selected
 * image's chain behind the gray one.  Going back to RTDD_GUIDE_GRAY keeps the allocation (asking for BGR again builds the chains again
 * from the images as they are).  A pyramid that never asks for BGR allocates nothing and launches nothing it did not launch before.
 * A logged estimate remembers the guide it ran with: a healed time-out runs it again with that guide, whatever the pyramid's is by then.
 * Refused: no pyramid (RTDD_ERR_STATE), an unknown kind.  rtdd_pyramid_guide: the guide in force (RTDD_GUIDE_GRAY without a pyramid). */
int rtdd_pyramid_set_guide(rtdd_ctx *ctx, int guideKind);
int rtdd_pyramid_guide(rtdd_ctx *ctx);
/* The depth regions of the pyramid's estimates (enum rtdd_region_flags and the rule: rtdd_solve_regions above).  The first call with
 * non-zero flags allocates, zeroed and per image of a batch, a second level-0 pair -- RTDD_IMG_REGION_EDITED, RTDD_IMG_REGION_MASK --
 * and one code plane per level, RTDD_IMG_REGION_CODE (RTDD_ERR_NOMEM: nothing is kept).  The pair is painted with the paint calls as they
 * are: rtdd_paint_image, rtdd_paint_strokes, rtdd_paint_ramp_strokes, rtdd_fill_polygon and rtdd_fill_similar given the pyramid's own
 * REGION pair as `edited` / `scribble` note a region change (where, given the annotation pair, they note an annotation change): the
 * label is the region id, an erased pixel or one painted with label 0 is unassigned, and the annotation is neither marked as changed
 * nor asked to be rebuilt.  rtdd_fill_similar's "similar" still reads the photograph passed as `original`.  rtdd_upload into the pair
 * notes the change too; a host that writes it by other means says so with rtdd_pyramid_regions_changed (RTDD_ERR_STATE without regions).
 * While the flags are non-zero, rtdd_estimate_depth, rtdd_estimate_depth_batch, rtdd_live_submit / _ex and rtdd_refine_depth first fill
 * every level's code plane from the pair when it changed (one launch: rtdd_region_codes' rule for every level and every image of a
 * batch), then solve every level with that level's codes and the flags.  Independent of rtdd_pyramid_set_guide: all four combinations
 * work.  Flags 0 switches the effect off and keeps the images, so a host can toggle before and after; a pyramid that never asks
 * allocates nothing and launches nothing it did not launch before.  rtdd_pyramid_set_image makes the selected image's regions
 * unassigned again, like its annotation.  A logged estimate remembers the flags it ran with: a healed time-out runs it again with them.
 * Refused: no pyramid (RTDD_ERR_STATE), unknown flag bits.  rtdd_pyramid_regions: the flags in force (0 without a pyramid). */
int rtdd_pyramid_set_regions(rtdd_ctx *ctx, int flags);
int rtdd_pyramid_regions(rtdd_ctx *ctx);
int rtdd_pyramid_regions_changed(rtdd_ctx *ctx);
/* annotation: DEVICE pointer to a 1-channel u8 map; decode rule of src/main.cpp:160-168 (value != 32 -> label, mask 255) */
int rtdd_pyramid_set_annotation(rtdd_ctx *ctx, const uint8_t *annotation, size_t pitch);
int rtdd_pyramid_image(rtdd_ctx *ctx, int kind, int level, void **ptr, size_t *pitch, int *rows, int *cols);
/* The coarse annotation levels (GPUPyrDownAnnotation, src/main.cpp:249-253) and the coarsest level's injection (:257-259) are brought up
 * to date by the first rtdd_estimate_depth after the annotation changed, not by every estimate (they depend on nothing else, the
 * down-sampling only ever adds and the solver never moves a Dirichlet pixel: same images, same bits).  Every entry point of this
 * library that writes RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED (set_image, set_annotation, rtdd_paint_image, rtdd_paint_strokes,
 * rtdd_pyrdown_annotation, rtdd_upload) notes the change itself; a caller that writes those images, or the coarsest RTDD_IMG_DEPTH, through the raw
 * pointers by other means says so with this call. */
int rtdd_pyramid_annotation_changed(rtdd_ctx *ctx);
/* rtdd_pyramid_annotation_changed, and in addition: labels were REMOVED.  The coarse levels only ever accumulate (above), so a level-0
 * pixel cleared through the raw pointers, or a live frame that uploads a pair with fewer labels than the frame before, would leave its old
 * label as a Dirichlet value on every coarse level.  After this call the next estimate builds the coarse RTDD_IMG_SCRIBBLE /
 * RTDD_IMG_EDITED levels AS IF THEY HAD BEEN ALL ZERO (their state after rtdd_pyramid_create / _set_image) before the down-sampling of
 * src/main.cpp:249-253 and the coarsest injection (:257): one launch that stores every coarse pixel, every image of a batched pyramid,
 * anything written into the coarse levels by other means included.  RTDD_IMG_DEPTH is left alone: the coarsest level keeps its last result
 * as the warm start (the reference's behaviour between frames), erased pixels are simply free again.  A live host that erased on its side
 * calls this before the rtdd_live_submit that uploads the reduced pair; an erasing rtdd_paint_strokes on the pyramid's own images calls
 * it itself.  Every other call accumulates, as before.
 * Healing (RTDD_ERR_TIMEOUT): an estimate or live frame that rebuilt is run again WITH the rebuild, from the annotation pair it ran on, and
 * the accumulating frames run again behind it add their levels again -- a rebuilt frame's Dirichlet pixels are its own on every level,
 * whatever a newer frame in flight has added since, and with one frame in flight the replayed bits are the first run's.  (With a newer
 * frame in flight, that frame's labels may still sit in the coarsest RTDD_IMG_DEPTH as the warm-start values of pixels the older frame
 * leaves free; accumulating frames that are run again with no rebuilt frame in front of them may see a newer frame's coarse strokes, as
 * noted at rtdd_live_submit.) */
int rtdd_pyramid_annotation_rebuild(rtdd_ctx *ctx);
/* src/main.cpp:239-291; asynchronous; results in RTDD_IMG_DEPTH (all levels) and RTDD_IMG_DEPTH_U8 */
int rtdd_estimate_depth(rtdd_ctx *ctx, int maxIterations);
/* Live mode: one frame of src/main.cpp:232-295 as the reference clocks it -- upload of the host's scribble and edited images
 * (:236-237), the estimate, download of the u8 map (:290-291) -- pipelined two frames deep: the copies run on a second stream of the
 * context's, so frame N+1's upload and frame N's download overlap the other frame's arithmetic and a frame costs about
 * max(compute, copies).  rtdd_live_submit returns at once; the host buffers must stay valid (and unchanged) until the frame has been
 * waited for, and should be page-locked (rtdd_host_alloc) -- pageable memory makes the copies synchronous, and with no other frame in
 * flight a page-locked hostDepthU8 is written by the estimate's last kernel itself instead of being downloaded (RTDD_OPT_LIVE_ZERO_COPY);
 * otherwise rtdd_live_wait downloads the map.  hostScribble / hostEdited
 * NULL: no upload, the annotation is the one already on the device.  A third submit waits for the oldest frame itself.
 * rtdd_live_wait blocks until the OLDEST frame in flight has landed in its host buffer (a timed-out persistent launch is healed
 * there like in rtdd_ctx_synchronize: every frame in flight is run again on its own uploaded annotation; the COARSE annotation levels,
 * which only ever accumulate, may by then hold the newer frame's strokes too).  Results: hostDepthU8, and RTDD_IMG_DEPTH /
 * RTDD_IMG_DEPTH_U8 on the device as after rtdd_estimate_depth.  No staging copies: an uploaded annotation pair BECOMES the pyramid's
 * level-0 RTDD_IMG_SCRIBBLE / RTDD_IMG_EDITED -- pointers obtained from rtdd_pyramid_image for those two images are good until the
 * next rtdd_live_submit that uploads: ask again after it (every other image keeps its address; a library call handed such a retired
 * pointer -- rtdd_paint_image, rtdd_paint_strokes, rtdd_upload, rtdd_convert_to_float, rtdd_pyrdown_annotation -- fails with RTDD_ERR_STATE instead of
 * writing a buffer no estimate reads). */
int rtdd_live_submit(rtdd_ctx *ctx, const uint8_t *hostScribble, size_t scribblePitch, const uint8_t *hostEdited, size_t editedPitch,
                     int maxIterations, uint8_t *hostDepthU8, size_t depthPitch);
/* The reference's frame WITH a sticky depth effect (src/main.cpp:190-230: once 'b' / 'g' / 'h' has been pressed the effect is rendered
 * and its image downloaded in every iteration of the loop at :180, next to the estimate at :232).  rtdd_live_submit plus: `effect` is
 * rendered from the frame's own depth map (RTDD_IMG_ORIGINAL, RTDD_IMG_GRAY, RTDD_IMG_DEPTH level 0) by the effect's kernel queued
 * right behind the estimate's copy-back, and the artistic image lands in hostArtistic (u8 x 3, page-locked for an asynchronous copy)
 * by the time rtdd_live_wait returns for the frame: downloaded by rtdd_live_wait while the next frame computes when frames are
 * pipelined, queued on the compute stream when no other frame is in flight.  RTDD_IMG_ARTISTIC then names the newest frame's image
 * on the device (like the annotation pair: ask rtdd_pyramid_image again after a submit with an effect).  The reference renders the
 * effect at the TOP of the next loop iteration from the same depth map -- the same sequence of artistic images, shown one iteration
 * later.  RTDD_EFFECT_NONE: exactly rtdd_live_submit (hostArtistic ignored).  A healed time-out renders the effect again too. */
enum rtdd_effect { RTDD_EFFECT_NONE = 0, RTDD_EFFECT_DEFOCUS = 1, RTDD_EFFECT_DESATURATION = 2, RTDD_EFFECT_HAZE = 3 };
int rtdd_live_submit_ex(rtdd_ctx *ctx, const uint8_t *hostScribble, size_t scribblePitch, const uint8_t *hostEdited, size_t editedPitch,
                        int maxIterations, uint8_t *hostDepthU8, size_t depthPitch, int effect, uint8_t *hostArtistic, size_t artisticPitch);
int rtdd_live_wait(rtdd_ctx *ctx);
int rtdd_live_pending(rtdd_ctx *ctx);                    /* frames submitted and not yet waited for: 0..2 */
int rtdd_host_alloc(void **ptr, size_t bytes);           /* page-locked host memory (hipHostMalloc) / its release */
int rtdd_host_free(void *ptr);
/* Extension: one more solve of the finest level, in place on RTDD_IMG_DEPTH level 0, by rtdd_solve_ex with `params`
 * (e.g. RTDD_METHOD_RED_BLACK_GS + RTDD_RELAXATION_AUTO, or RTDD_METHOD_MULTIGRID, tolerance 1e-4), then RTDD_IMG_DEPTH_U8
 * again: "estimate, then converge".  The level-0 edge weights are rebuilt from the current depth, as every solve does
 * (src/GPUSolver.cu:136-224).  Synchronises when params->tolerance > 0. */
int rtdd_refine_depth(rtdd_ctx *ctx, const rtdd_solve_params *params, rtdd_solve_info *info);
/* the standalone third-party pieces, exposed for parity tests against the oracle's restatement */
int rtdd_bgr2gray(rtdd_ctx *ctx, const uint8_t *bgr, size_t bgrPitch, uint8_t *gray, size_t grayPitch, int rows, int cols);
int rtdd_pyrdown_gray(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, int rows, int cols, uint8_t *dst, size_t dstPitch);
/* rtdd_pyrdown_gray on each channel of an interleaved u8x3 image (dst: (rows + 1) / 2 x (cols + 1) / 2, dstPitch >= 3 * that width) */
int rtdd_pyrdown_bgr(rtdd_ctx *ctx, const uint8_t *src, size_t srcPitch, int rows, int cols, uint8_t *dst, size_t dstPitch);
int rtdd_pyrup_depth(rtdd_ctx *ctx, const float *src, size_t srcPitch, int rows, int cols,
                     float *dst, size_t dstPitch, int dstRows, int dstCols);
int rtdd_depth_to_u8(rtdd_ctx *ctx, const float *src, size_t srcPitch, uint8_t *dst, size_t dstPitch, int rows, int cols);
/* pitched host<->device copies on the context's stream, then a stream sync (harness / binding convenience).  Any host pitch: a
 * contiguous host image whose pitch is no multiple of four (an odd-width cv::Mat) goes as one linear copy through a device buffer --
 * the runtime's own 2-D copy takes ~9 us per row for such a pitch.  rtdd_live_submit's copies do the same. */
int rtdd_upload(rtdd_ctx *ctx, void *dev, size_t devPitch, const void *host, size_t hostPitch, size_t widthBytes, int rows);
int rtdd_download(rtdd_ctx *ctx, void *host, size_t hostPitch, const void *dev, size_t devPitch, size_t widthBytes, int rows);

/* ---- instrumentation ------------------------------------------------------------------------ */

/* Device time of the solver's phases, measured with HIP events recorded on the context's stream around
 * them (enable with rtdd_profile_enable(ctx, 1)).  Recording does not synchronise; rtdd_profile_get waits
 * for the recorded calls and returns TOTALS over the solve calls made since the previous rtdd_profile_get
 * (at most the last 64).  launches = sweep-kernel launches, sweeps = Jacobi sweeps they performed. */
typedef struct rtdd_profile {
    double sweep_ms;
    int launches;
    int sweeps;
    double prepare_ms;              /* edge-weight + staging pass */
    double finish_ms;               /* copy back to the caller's pitched buffer */
} rtdd_profile;
int rtdd_profile_enable(rtdd_ctx *ctx, int on);
int rtdd_profile_get(rtdd_ctx *ctx, rtdd_profile *out);

#ifdef __cplusplus
}
#endif
#endif /* RTDD_H */
