// api.cpp -- the core of the extern "C" surface of librtdd.so (include/rtdd.h): context, option table, profile, rtdd_allocate /
// rtdd_load_weights, the per-level solve driver (GPUMatrixFreeSolver, /root/reference/src/GPUSolver.cu:274-316) with the solve entry
// points.  The pending-call log and its replay: heal.cpp; the depth effects: effects_api.cpp; the calls on images they are handed:
// image_api.cpp; the pyramid, the whole estimate, live mode: pyramid.cpp, estimate.cpp, live.cpp.  Host code only; kernels: *.hip.
#include <climits>
#include <cmath>
#include <cstring>
#include <new>

#include "rtdd_internal.hpp"
#include "persist_sync.hpp"

namespace rtdd {

int fail(rtdd_ctx *ctx, int status, const char *what, hipError_t e) {
    if (ctx) {
        ctx->last_error = what ? what : "";
        if (e != hipSuccess) {
            ctx->last_error += ": ";
            ctx->last_error += hipGetErrorString(e);
        }
    }
    return status;
}

// omega recurrence of the reference driver (src/GPUSolver.cu:282-299): float state, double
// intermediates, S = 10, rho = 0.99f.
void omega_schedule(int n, std::vector<float> &out) {
    out.resize(n > 0 ? n : 0);
    const int S = 10;
    float omega = 0.0f;
    const float rho = 0.99;
    for (int it = 0; it < n; it++) {
        if (it < S) omega = 1;
        else if (it == S) omega = 2.0 / (2.0 - rho * rho);
        else omega = 4.0 / (4.0 - rho * rho * omega);
        out[it] = omega;
    }
}

static void free_levels(rtdd_ctx *ctx) {
    for (auto &L : ctx->levels) {
        for (auto &p : L.plane)
            if (p) { (void)hipFree(p); p = nullptr; }
        if (L.meta) { (void)hipFree(L.meta); L.meta = nullptr; }
    }
    ctx->levels.clear();
    ctx->maxLevel = -1;
}

}  // namespace rtdd

using namespace rtdd;

#pragma GCC visibility push(default)
extern "C" {

int rtdd_version(void) { return RTDD_VERSION; }

const char *rtdd_status_string(int s) {
    switch (s) {
        case RTDD_OK: return "ok";
        case RTDD_ERR_INVALID: return "invalid argument";
        case RTDD_ERR_STATE: return "call order violated";
        case RTDD_ERR_HIP: return "HIP runtime error";
        case RTDD_ERR_NOMEM: return "out of memory";
        case RTDD_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
        case RTDD_ERR_TIMEOUT: return "persistent kernel timed out (workgroups not co-resident)";
        default: return "unknown status";
    }
}

const char *rtdd_last_error(rtdd_ctx *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int rtdd_ctx_create(int device, rtdd_ctx **out) {
    if (!out) return RTDD_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RTDD_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RTDD_ERR_INVALID;
    rtdd_ctx *ctx = new (std::nothrow) rtdd_ctx();
    if (!ctx) return RTDD_ERR_NOMEM;
    ctx->device = device;
    for (auto &t : ctx->persist_fit) t[0] = t[1] = -1;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    bool ok = hipMalloc((void **)&ctx->lut_dev, 257 * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&ctx->residual_dev, 64) == hipSuccess &&
              hipMalloc((void **)&ctx->sync_words, kSyncWords * sizeof(int)) == hipSuccess &&
              hipMemset(ctx->sync_words, 0, kSyncWords * sizeof(int)) == hipSuccess;
    for (auto &e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    // the word the copy-back kernels report confirmed solves in: page-locked host memory the device writes directly (persist_sync.hpp)
    if (ok && hipHostMalloc((void **)&ctx->confirm_host, 64, hipHostMallocMapped) == hipSuccess) {
        *ctx->confirm_host = 0;
        void *dev_view = nullptr;
        ok = hipHostGetDevicePointer(&dev_view, ctx->confirm_host, 0) == hipSuccess &&
             hipMemcpy(ctx->sync_words + kSyncConfirmPtr, &dev_view, sizeof(dev_view), hipMemcpyHostToDevice) == hipSuccess;
    } else ok = false;
    if (!ok) { rtdd_ctx_destroy(ctx); return RTDD_ERR_HIP; }
    *out = ctx;
    return RTDD_OK;
}

int rtdd_ctx_destroy(rtdd_ctx *ctx) {
    if (!ctx) return RTDD_OK;
    DeviceGuard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    pyramid_free(ctx);
    mg_release(ctx);
    free_levels(ctx);
    if (ctx->lut_dev) (void)hipFree(ctx->lut_dev);
    if (ctx->omega_dev) (void)hipFree(ctx->omega_dev);
    if (ctx->residual_dev) (void)hipFree(ctx->residual_dev);
    if (ctx->sync_words) (void)hipFree(ctx->sync_words);
    if (ctx->sat) (void)hipFree(ctx->sat);
    if (ctx->bounce.ptr) (void)hipFree(ctx->bounce.ptr);
    if (ctx->confirm_host) (void)hipHostFree(ctx->confirm_host);
    for (auto &e : ctx->ev) if (e) (void)hipEventDestroy(e);
    delete ctx;
    return RTDD_OK;
}

int rtdd_ctx_set_stream(rtdd_ctx *ctx, rtdd_stream stream) {
    if (!ctx) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    // the logged calls were queued on the OLD stream: confirm (or heal) them there before anything is queued on the new one
    RTDD_TRY(settle_pending(ctx));
    ctx->stream = (hipStream_t)stream;
    return RTDD_OK;
}

int rtdd_ctx_synchronize(rtdd_ctx *ctx) {
    if (!ctx) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // (a timed-out persistent launch is healed here: the affected calls run again, heal.cpp)
    return check_persistent_status(ctx);
}

// One row per settable option: the Options member it reads and writes, the admitted range and the refusal text; zero_or_one: any value
// is admitted and stored as 0 or 1.  (The read-only keys are rtdd_get_option's own: a set finds no row for them.)
static const struct OptionRow {
    int key;
    int Options::*member;
    bool zero_or_one;
    int lo, hi; const char *refusal;
} kOptions[] = {
    {RTDD_OPT_FP_CONTRACT, &Options::fp_contract, true, 0, 1, nullptr},
    {RTDD_OPT_SWEEP_KERNEL, &Options::sweep_kernel, false, 0, 2, "sweep kernel must be 0..2"},
    {RTDD_OPT_TEMPORAL_DEPTH, &Options::temporal_depth, false, 0, 28, "temporal depth must be 0..28"},
    {RTDD_OPT_ROWS_PER_WAVE, &Options::rows_per_wave, false, 0, 1024, "rows per wave must be 0..1024"},
    {RTDD_OPT_DEFOCUS_PATH, &Options::defocus_path, false, 0, 2, "defocus path must be 0..2"},
    {RTDD_OPT_TILE, &Options::tile, false, 0, 16, "tile must be 0..16"},
    {RTDD_OPT_PERSISTENT, &Options::persistent, true, 0, 1, nullptr},
    {RTDD_OPT_ANNOTATION_LDS, &Options::annotation_lds, true, 0, 1, nullptr},
    {RTDD_OPT_LIVE_ZERO_COPY, &Options::live_zero_copy, false, 0, 2, "RTDD_OPT_LIVE_ZERO_COPY is 0, 1 or 2"},
    {RTDD_OPT_TIMEOUT_HEAL, &Options::timeout_heal, true, 0, 1, nullptr},
    {RTDD_OPT_PERSISTENT_REARM_AFTER, &Options::rearm_after, false, 0, 1 << 20, "must be 0..2^20"},
    {RTDD_OPT_DEFOCUS_SLICE_MB, &Options::defocus_slice_mb, false, 0, 4095, "must be 0..4095 MB"},
    {RTDD_OPT_DEFOCUS_STRIPS, &Options::defocus_strips, false, 0, 2, "must be 0, 1 or 2"},
    {RTDD_OPT_AUTO_CYCLE_FIXED_NS, &Options::auto_cycle_fixed_ns, false, 0, INT_MAX, "must be >= 0"},
    {RTDD_OPT_AUTO_CYCLE_FS_PER_PX, &Options::auto_cycle_fs_per_px, false, 0, INT_MAX, "must be >= 0"},
    {RTDD_OPT_AUTO_SWEEP_FS_PER_PX, &Options::auto_sweep_fs_per_px, false, 0, INT_MAX, "must be >= 0"},
    {RTDD_OPT_AUTO_SWEEP_FLOOR_NS, &Options::auto_sweep_floor_ns, false, 0, INT_MAX, "must be >= 0"},
    {RTDD_OPT_DEBUG_WITHHOLD_TILE, &Options::debug_withhold_tile, false, 0, kSyncMaxTiles, "tile number + 1 out of range"},
    {RTDD_OPT_DEBUG_POLL_LIMIT_US, &Options::debug_poll_limit_us, false, 0, 10000000, "poll limit must be 0..1e7 us"},
    {RTDD_OPT_DEBUG_FORCE_STATUS, &Options::debug_force_status, false, 0, 3, "status must be 0..3"},
};
static const OptionRow *find_option(int key) {
    for (const OptionRow &r : kOptions) if (r.key == key) return &r;
    return nullptr;
}

int rtdd_set_option(rtdd_ctx *ctx, int key, int value) {
    if (!ctx) return RTDD_ERR_INVALID;
    const OptionRow *r = find_option(key);
    if (!r) return fail(ctx, RTDD_ERR_INVALID, "unknown option");
    if (r->zero_or_one) value = value ? 1 : 0;
    else REQUIRE(ctx, value >= r->lo && value <= r->hi, r->refusal);
    ctx->opt.*(r->member) = value;
    switch (key) {                      // the setters that do more than store
        // (setting the automatic choice again forgets what earlier depths made it choose)
        case RTDD_OPT_DEFOCUS_PATH: if (value == 0) ctx->defocus_table_sticky = ctx->defocus_band_sticky = false; break;
        // (said explicitly: armed at once, whatever a heal suspended)
        case RTDD_OPT_PERSISTENT: ctx->persistent_wanted = value; ctx->persist_suspend = 0; break;
        case RTDD_OPT_TIMEOUT_HEAL: if (!value && !ctx->healing) { ctx->pending.clear(); ctx->pending_overflow = false; } break;
        default: break;
    }
    return RTDD_OK;
}

int rtdd_get_option(rtdd_ctx *ctx, int key, int *value) {
    if (!ctx || !value) return RTDD_ERR_INVALID;
    if (const OptionRow *r = find_option(key)) { *value = ctx->opt.*(r->member); return RTDD_OK; }
    switch (key) {                      // read only
        case RTDD_OPT_TIMEOUT_HEALS: *value = ctx->heals; break;
        case RTDD_OPT_DEFOCUS_LAST_PATH: *value = ctx->defocus_last_path; break;
        case RTDD_OPT_DEFOCUS_LAST_SLICES: *value = ctx->defocus_last_slices; break;
        case RTDD_OPT_PERSISTENT_SUSPENDED: *value = ctx->persist_suspend; break;
        case RTDD_OPT_PENDING_CALLS: prune_confirmed(ctx); *value = (int)ctx->pending.size(); break;
        default: return fail(ctx, RTDD_ERR_INVALID, "unknown option");
    }
    return RTDD_OK;
}

int rtdd_profile_enable(rtdd_ctx *ctx, int on) {
    if (!ctx) return RTDD_ERR_INVALID;
    ctx->profile_on = on != 0;
    ctx->prof_pending = 0;
    return RTDD_OK;
}

int rtdd_profile_get(rtdd_ctx *ctx, rtdd_profile *out) {
    if (!ctx || !out) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    // totals over the solve calls made since the previous rtdd_profile_get (at most the last kProfSlots of them)
    rtdd_profile p{};
    const int n = ctx->prof_pending < rtdd_ctx::kProfSlots ? ctx->prof_pending : rtdd_ctx::kProfSlots;
    for (int i = 0; i < n; i++) {
        const int slot = (ctx->prof_pending - 1 - i) % rtdd_ctx::kProfSlots;
        hipEvent_t *ev = ctx->ev + 4 * slot;
        RTDD_HIP(ctx, hipEventSynchronize(ev[3]));
        float a = 0, b = 0, c = 0;
        RTDD_HIP(ctx, hipEventElapsedTime(&a, ev[0], ev[1]));
        RTDD_HIP(ctx, hipEventElapsedTime(&b, ev[1], ev[2]));
        RTDD_HIP(ctx, hipEventElapsedTime(&c, ev[2], ev[3]));
        p.prepare_ms += a; p.sweep_ms += b; p.finish_ms += c;
        p.launches += ctx->prof_launches[slot]; p.sweeps += ctx->prof_sweeps[slot];
    }
    ctx->prof_pending = 0;
    ctx->prof = p;
    *out = p;
    return RTDD_OK;
}

// ---- solver ------------------------------------------------------------------------------------

int rtdd_allocate(rtdd_ctx *ctx, int rows, int cols, int levels) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, rows > 0 && cols > 0 && levels > 0 && levels <= 30, "rows, cols, levels must be positive");
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_levels(ctx);
    const int images = ctx->alloc_images > 0 ? ctx->alloc_images : 1;
    ctx->alloc_images = 1;                         // (one shot: rtdd_pyramid_create_batch sets it for the call it makes)
    ctx->levels.resize(levels);
    for (int l = 0; l < levels; l++) {
        Level &L = ctx->levels[l];
        L.rows = (int)(rows / powf(2, l));          // src/GPUSolver.cu:42-43 (float divide, truncation)
        L.cols = (int)(cols / powf(2, l));
        L.elems = plane_elems(L.rows > 0 ? L.rows : 1, L.cols > 0 ? L.cols : 1);
        const size_t all = L.elems * (size_t)images;           // (a batched pyramid: every plane once per image, Level::view)
        for (auto &p : L.plane) {
            hipError_t e = hipMalloc((void **)&p, all * sizeof(float));
            if (e != hipSuccess) { free_levels(ctx); return fail(ctx, e == hipErrorOutOfMemory ? RTDD_ERR_NOMEM : RTDD_ERR_HIP,
                "hipMalloc(plane)", e); }
        }
        hipError_t e = hipMalloc((void **)&L.meta, all * sizeof(uint32_t));
        if (e != hipSuccess) { free_levels(ctx); return fail(ctx, e == hipErrorOutOfMemory ? RTDD_ERR_NOMEM : RTDD_ERR_HIP,
            "hipMalloc(meta)", e); }
        // guard cells are read (never used); give them a defined value once
        for (auto &p : L.plane) RTDD_HIP(ctx, hipMemsetAsync(p, 0, all * sizeof(float), ctx->stream));
        RTDD_HIP(ctx, hipMemsetAsync(L.meta, 0, all * sizeof(uint32_t), ctx->stream));
    }
    ctx->levels_images = images;
    ctx->maxLevel = levels - 1;                    // :51
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the reference syncs here (:52)
    return RTDD_OK;
}

int rtdd_free(rtdd_ctx *ctx) {
    if (!ctx) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    mg_release(ctx);
    free_levels(ctx);
    return RTDD_OK;
}

int rtdd_load_weights(rtdd_ctx *ctx, float beta) {
    if (!ctx) return RTDD_ERR_INVALID;
    DeviceGuard g(ctx->device);
    RTDD_TRY(settle_pending(ctx));
    for (int w = 0; w < 256; w++) ctx->lut_host[w] = expf(-beta * w);      // src/GPUSolver.cu:267, host libm
    ctx->lut_host[256] = 0;
    RTDD_HIP(ctx, hipMemcpyAsync(ctx->lut_dev, ctx->lut_host, sizeof(ctx->lut_host), hipMemcpyHostToDevice, ctx->stream));
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));                      // lut_host may be rewritten by the next call
    ctx->weights_loaded = true;
    return RTDD_OK;
}

// The omega schedule depends only on the iteration index, so one device copy serves every call;
// it is re-uploaded only when a longer schedule is requested.
static int ensure_omegas(rtdd_ctx *ctx, int n) {
    if (n <= ctx->omega_cap) return RTDD_OK;
    int cap = n < 1024 ? 1024 : n;
    std::vector<float> om;
    omega_schedule(cap, om);
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->omega_dev) { RTDD_HIP(ctx, hipFree(ctx->omega_dev)); ctx->omega_dev = nullptr; ctx->omega_cap = 0; }
    RTDD_HIP(ctx, hipMalloc((void **)&ctx->omega_dev, (size_t)cap * sizeof(float)));
    RTDD_HIP(ctx, hipMemcpy(ctx->omega_dev, om.data(), (size_t)cap * sizeof(float), hipMemcpyHostToDevice));
    ctx->omega_cap = cap;
    return RTDD_OK;
}

static constexpr int kAutoMaxCycles = 60;

static int check_solve_args(rtdd_ctx *ctx, const SolveCall &c) {
    REQUIRE(ctx, c.depth && c.scribble && c.gray, "null image pointer");
    REQUIRE(ctx, c.rows > 0 && c.cols > 0, "rows and cols must be positive");
    REQUIRE(ctx, f32_image_aligned(c.depth, c.depthPitch), kF32AlignText);
    REQUIRE(ctx, c.depthPitch >= (size_t)c.cols * sizeof(float), "depth pitch smaller than a row");
    REQUIRE(ctx, c.guide == RTDD_GUIDE_GRAY || c.guide == RTDD_GUIDE_BGR, "unknown guide kind");
    REQUIRE(ctx, c.scribblePitch >= (size_t)c.cols && c.grayPitch >= (size_t)c.cols * (c.guide == RTDD_GUIDE_BGR ? 3 : 1), "u8 pitch smaller than a row");
    REQUIRE(ctx, (c.regionFlags & ~(RTDD_REGION_CUT | RTDD_REGION_SMOOTH)) == 0, "unknown region flag");
    REQUIRE(ctx, c.regionFlags == 0 || (c.regions && c.regionsPitch >= (size_t)c.cols), "region flags without a region image, or its pitch smaller than a row");
    if (ctx->levels.empty()) return fail(ctx, RTDD_ERR_STATE, "rtdd_allocate has not been called");
    if (!ctx->weights_loaded) return fail(ctx, RTDD_ERR_STATE, "rtdd_load_weights has not been called");
    REQUIRE(ctx, c.level >= 0 && c.level < (int)ctx->levels.size(), "level out of range");
    const Level &L = ctx->levels[c.level];
    REQUIRE(ctx, plane_elems(c.rows, c.cols) <= L.elems, "rows x cols exceeds the level's allocation");
    return RTDD_OK;
}

namespace {

// One rtdd_solve_ex call between k_prepare and k_finish: which planes hold the iterate, what has run, the last residual.
struct Solve {
    rtdd_ctx *ctx;
    const Level &L;
    size_t ip;
    int rows, cols;
    const rtdd_solve_params *p;
    int images;                                    // a batched solve: the images every launch covers (blockIdx.z)
    int done = 0, launches = 0, cycles = 0;
    int pk = 0, pm = 1;                            // planes holding x_k and x_{k-1}
    float residual = NAN;

    bool stop_on_residual() const { return p->tolerance > 0.0f; }
    bool reached() const { return residual <= p->tolerance; }
    int check() { return launch_residual(ctx, L, ip, pk, rows, cols, &residual); }

    // the reference's scheme, optionally in chunks with a residual check after each
    int chebyshev_jacobi() {
        std::vector<float> omegas;
        omega_schedule(p->maxIterations, omegas);
        const bool blocked = ctx->opt.sweep_kernel != 1;       // 0 (auto) and 2 -> temporally blocked kernel
        const float *omegas_dev = nullptr;
        int rc;
        if (blocked && p->maxIterations > 0) {
            if ((rc = ensure_omegas(ctx, p->maxIterations)) != RTDD_OK) return rc;
            omegas_dev = ctx->omega_dev;
        }
        const int chunk = stop_on_residual() ? (p->checkEvery > 0 ? p->checkEvery : 16) : p->maxIterations;
        while (done < p->maxIterations) {
            const int n = p->maxIterations - done < chunk ? p->maxIterations - done : chunk;
            int ln = 0;
            rc = blocked ? launch_sweeps_blocked(ctx, L, ip, rows, cols, omegas_dev + done, n, &pk, &pm, &ln, images)
                         : launch_sweeps(ctx, L, ip, rows, cols, omegas.data() + done, n, &pk, &pm, &ln);
            if (rc != RTDD_OK) return rc;
            done += n; launches += ln;
            if (stop_on_residual()) {
                if ((rc = check()) != RTDD_OK) return rc;
                if (reached()) break;
            }
        }
        return RTDD_OK;
    }

    // n red-black sweeps (capped by maxIterations) at one relaxation factor
    int red_black_sweeps(int n, float omega) {
        if (n > p->maxIterations - done) n = p->maxIterations - done;
        if (n <= 0) return RTDD_OK;
        int ln = 2 * n, rc;
        if (ctx->opt.sweep_kernel == 1) rc = launch_rbgs(ctx, L, ip, pk, rows, cols, n, omega);     // one launch per colour, in place
        else rc = launch_rbgs_blocked(ctx, L, ip, rows, cols, n, omega, &pk, &ln);                  // register-blocked, ping-pong planes
        done += n; launches += ln;
        return rc;
    }

    // Gauss-Seidel / SOR at a fixed factor, optionally in chunks with a residual check after each
    int red_black() {
        const int chunk = stop_on_residual() ? (p->checkEvery > 0 ? p->checkEvery : 16) : (p->maxIterations > 0 ? p->maxIterations : 1);
        const float omega = p->relaxation == 0.0f ? 1.0f : p->relaxation;
        int rc;
        while (done < p->maxIterations) {
            if ((rc = red_black_sweeps(chunk, omega)) != RTDD_OK) return rc;
            if (stop_on_residual()) {
                if ((rc = check()) != RTDD_OK) return rc;
                if (reached()) break;
            }
        }
        return RTDD_OK;
    }

    // RTDD_RELAXATION_AUTO: SOR cycles.  Over-relaxation removes the smooth error a plain sweep hardly touches, but in f32 it idles
    // at a residual ~ ulp(x)/(2 - omega); plain Gauss-Seidel has an exact f32 fixed point but is slow on smooth error.  So:
    // n_hi sweeps at omega_hi, n_hi/4 at omega_mid, then a Gauss-Seidel polish of at most 100 sweeps with the residual checked
    // every 20; a cycle that does not get there is followed by one twice as long and twice as close to omega = 2, until the
    // tolerance or maxIterations.  After V-cycles the smooth error is gone and half the length does
    // (scripts/auto_probe.py).
    int sor_cycles(bool after_vcycles) {
        const int longest = rows > cols ? rows : cols;
        const int base = after_vcycles ? (longest + 1) / 2 : longest;
        double w0 = 2.0 / (1.0 + sin(4.0 * 3.14159265358979323846 / (double)longest));
        if (w0 > 1.99) w0 = 1.99;
        if (w0 < 1.0) w0 = 1.0;
        bool ok = false;
        int rc;
        for (int cycle = 0; done < p->maxIterations && !ok; cycle++) {
            const int e = cycle < 6 ? cycle : 6;
            double gap = (2.0 - w0) / (double)(1 << e);
            if (gap < 0.005) gap = 0.005;
            const float w_hi = (float)(2.0 - gap);
            float w_mid = (float)(2.0 - 10.0 * gap);
            if (w_mid < 1.0f) w_mid = 1.0f;
            const int n_hi = base << e;
            if ((rc = red_black_sweeps(n_hi, w_hi)) != RTDD_OK) return rc;
            if ((rc = red_black_sweeps(n_hi / 4, w_mid)) != RTDD_OK) return rc;
            for (int k = 0; k < 5 && done < p->maxIterations && !ok; k++) {
                if ((rc = red_black_sweeps(20, 1.0f)) != RTDD_OK) return rc;
                if (stop_on_residual()) {
                    if ((rc = check()) != RTDD_OK) return rc;
                    ok = reached();
                }
            }
        }
        return RTDD_OK;
    }

    // V-cycles; alternative_seconds > 0: leave when the cycles still needed are modelled dearer than that (RTDD_METHOD_AUTO)
    int vcycles(int max_cycles, int check_every, double alternative_seconds) {
        const double px = (double)rows * cols;
        const double cycle_seconds = ctx->opt.auto_cycle_fixed_ns * 1e-9 + px * ctx->opt.auto_cycle_fs_per_px * 1e-15;
        return launch_multigrid(ctx, L, ip, rows, cols, max_cycles, p->tolerance, check_every, alternative_seconds, cycle_seconds, &pk,
            &cycles, &residual, &launches);
    }

    // V-cycles while they pay: they stop at the tolerance, after kAutoMaxCycles, or when the cycles still needed (at the rate of the
    // last two) are modelled to cost more than finishing with SOR cycles of half length -- thin high-contrast structures stall them
    // (DESIGN.md section 7), and below ~4K a cycle is launch-bound and dear.  Then those SOR cycles.
    int automatic() {
        const int longest = rows > cols ? rows : cols;
        const double px = (double)rows * cols;
        const double per_px = px * ctx->opt.auto_sweep_fs_per_px * 1e-15, floor_s = ctx->opt.auto_sweep_floor_ns * 1e-9;
        const double sweep_seconds = per_px > floor_s ? per_px : floor_s;                   // k_rbgs_blocked (constants: RTDD_OPT_AUTO_*)
        const double sor_seconds = ((double)((longest + 1) / 2) * 1.25 + 20.0) * sweep_seconds;
        const int rc = vcycles(kAutoMaxCycles, 1, sor_seconds);
        if (rc != RTDD_OK || reached()) return rc;
        return sor_cycles(true);
    }
};

}  // namespace

// one attempt: stage + edge weights, the sweeps, the (guarded) copy-back
static int solve_once(rtdd_ctx *ctx, const SolveCall &c, int seq, SolveOutcome *out) {
    const SolveTargets &t = c.targets;
    // (the first image the launches cover: image 0 of 1 unless the caller says otherwise)
    const Level L = ctx->levels[c.level].view(t.batch.first);
    const size_t ip = plane_pitch(c.cols);
    const bool prof = ctx->profile_on;
    hipEvent_t *ev = ctx->ev + 4 * (ctx->prof_pending % rtdd_ctx::kProfSlots);

    if (prof) RTDD_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    ctx->wild_seq = seq;                           // k_prepare tags depths outside the fast divide's domain with it; the sweep kernels compare (persist_sync.hpp kSyncWild)
    int rc = launch_prepare(ctx, L, ip, c);
    if (rc != RTDD_OK) return rc;
    if (prof) RTDD_HIP(ctx, hipEventRecord(ev[1], ctx->stream));

    ctx->last_info = rtdd_solve_info{};
    ctx->last_info.residual = NAN;
    Solve s{ctx, L, ip, c.rows, c.cols, &c.params, t.batch.n};
    switch (c.params.method) {
        case RTDD_METHOD_CHEBYSHEV_JACOBI: rc = s.chebyshev_jacobi(); break;
        case RTDD_METHOD_MULTIGRID:
            rc = s.vcycles(c.params.maxIterations, c.params.checkEvery > 0 ? c.params.checkEvery : 1, 0.0);
            s.done = s.cycles;
            break;
        case RTDD_METHOD_AUTO: rc = s.automatic(); break;
        default: rc = c.params.relaxation < 0.0f ? s.sor_cycles(false) : s.red_black(); break;
    }
    if (rc != RTDD_OK) return rc;

    if (prof) RTDD_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    // (a deferred copy-back is k_pyrup_inject's: estimate_levels hands it the same number)
    if (out) { out->plane = s.pk; out->seq = seq; }
    if (!t.defer_finish) {
        rc = launch_finish(ctx, L, ip, s.pk, c, seq);
        if (rc != RTDD_OK) return rc;
    }
    if (prof) {
        RTDD_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
        const int slot = ctx->prof_pending % rtdd_ctx::kProfSlots;
        ctx->prof_launches[slot] = s.launches; ctx->prof_sweeps[slot] = s.done;
        ctx->prof_pending++;                        // resolved (and synchronised) by rtdd_profile_get, not here
    }
    ctx->last_info.iterations = s.done; ctx->last_info.residual = s.residual; ctx->last_info.cycles = s.cycles;
    ctx->last_info.fp_contract = ctx->opt.fp_contract; ctx->last_info.launches = s.launches;
    return RTDD_OK;
}

int rtdd_solve_ex(rtdd_ctx *ctx, float *depth, size_t depthPitch, const uint8_t *scribble, size_t scribblePitch,
                  const uint8_t *gray, size_t grayPitch, int rows, int cols, int level,
                  const rtdd_solve_params *params, rtdd_solve_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, params != nullptr, "null params");
    return solve_with(ctx, {depth, depthPitch, scribble, scribblePitch, gray, grayPitch, RTDD_GUIDE_GRAY, rows, cols, level, *params, {}}, info, nullptr);
}

int rtdd_solve_guided(rtdd_ctx *ctx, float *depth, size_t depthPitch, const uint8_t *scribble, size_t scribblePitch,
                      const uint8_t *guide, size_t guidePitch, int guideKind, int rows, int cols, int level,
                      const rtdd_solve_params *params, rtdd_solve_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, params != nullptr, "null params");
    return solve_with(ctx, {depth, depthPitch, scribble, scribblePitch, guide, guidePitch, guideKind, rows, cols, level, *params, {}}, info, nullptr);
}

// rtdd_solve_guided with depth regions.  No regions, or flags 0, is rtdd_solve_guided: the record then holds neither
int rtdd_solve_regions(rtdd_ctx *ctx, float *depth, size_t depthPitch, const uint8_t *scribble, size_t scribblePitch,
                       const uint8_t *guide, size_t guidePitch, int guideKind, const uint8_t *regions, size_t regionsPitch, int regionFlags,
                       int rows, int cols, int level, const rtdd_solve_params *params, rtdd_solve_info *info) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, params != nullptr, "null params");
    REQUIRE(ctx, (regionFlags & ~(RTDD_REGION_CUT | RTDD_REGION_SMOOTH)) == 0, "unknown region flag");
    REQUIRE(ctx, regions || regionFlags == 0, "region flags without a region image");
    REQUIRE(ctx, !regions || cols <= 0 || regionsPitch >= (size_t)cols, "region pitch smaller than a row");
    SolveCall c{depth, depthPitch, scribble, scribblePitch, guide, guidePitch, guideKind, rows, cols, level, *params, {}};
    if (regions && regionFlags != 0) { c.regions = regions; c.regionsPitch = regionsPitch; c.regionFlags = regionFlags; }
    return solve_with(ctx, c, info, nullptr);
}

}  // extern "C"
#pragma GCC visibility pop

// rtdd_solve_ex, plus what the library's own callers add to it (SolveTargets: a batch of images in the same launches, a deferred
// copy-back, the u8 copies of the result, whether the call is logged on its own).
int rtdd::solve_with(rtdd_ctx *ctx, const SolveCall &c, rtdd_solve_info *info, SolveOutcome *out) {
    if (!ctx) return RTDD_ERR_INVALID;
    const SolveTargets &t = c.targets;
    REQUIRE(ctx, c.params.maxIterations >= 0, "maxIterations must be >= 0");
    REQUIRE(ctx, c.params.method == RTDD_METHOD_CHEBYSHEV_JACOBI || c.params.method == RTDD_METHOD_RED_BLACK_GS ||
                 c.params.method == RTDD_METHOD_MULTIGRID || c.params.method == RTDD_METHOD_AUTO, "unknown method");
    REQUIRE(ctx, c.params.method != RTDD_METHOD_AUTO || c.params.tolerance > 0.0f, "RTDD_METHOD_AUTO needs a tolerance");
    REQUIRE(ctx, c.params.method != RTDD_METHOD_RED_BLACK_GS || c.params.relaxation == RTDD_RELAXATION_AUTO ||
                 (c.params.relaxation >= 0.0f && c.params.relaxation < 2.0f), "relaxation must be in [0,2) or RTDD_RELAXATION_AUTO");
    RTDD_TRY(check_solve_args(ctx, c));
    REQUIRE(ctx, t.batch.first >= 0 && t.batch.n >= 1 && t.batch.first + t.batch.n <= ctx->levels_images,
            "the batch exceeds what the context's levels were allocated for");
    REQUIRE(ctx, t.batch.n == 1 || (c.params.method == RTDD_METHOD_CHEBYSHEV_JACOBI && c.params.tolerance <= 0.0f && ctx->opt.sweep_kernel != 1),
            "a batched solve runs the reference's scheme with the temporally blocked kernel only");
    DeviceGuard g(ctx->device);
    // (once in 10^9 solves) the sequence numbers start over: nothing may be left that compares against them
    if (ctx->solve_seq >= (1 << 30)) {
        if (!ctx->healing) RTDD_TRY(settle_pending(ctx));
        RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *(volatile int *)ctx->confirm_host = 0;
        RTDD_HIP(ctx, hipMemset(ctx->sync_words + kSyncWild, 0, 2 * sizeof(int)));      // (kSyncWild and kSyncLarge)
        ctx->solve_seq = 0; ctx->publish_seq = 0;
    }
    const int seq = ++ctx->solve_seq;
    const Options asked = ctx->opt;
    int rc = solve_once(ctx, c, seq, out);
    // A residual check inside the solve found the status word set, and the calls before this one have been healed
    // (check_persistent_status): nothing of this solve has reached the caller's buffers (its copy-back is the last thing it does), so
    // it simply starts over -- persistence is off by now.
    if (rc == kRestartSolve) rc = solve_once(ctx, c, seq, out);
    if (rc == kRestartSolve) rc = fail(ctx, RTDD_ERR_TIMEOUT, "the solve was restarted after a timed-out persistent launch and failed again");
    if (rc != RTDD_OK) return rc;
    // re-armed (check_persistent_status)
    if (!ctx->healing && ctx->persist_suspend > 0 && --ctx->persist_suspend == 0 && ctx->persistent_wanted) ctx->opt.persistent = 1;
    // remembered until a copy-back kernel or a synchronising call has confirmed it
    if (t.logged) {
        PendingOp op;
        op.kind = PendingOp::kSolve; op.opt = asked; op.solve = c; op.seq = seq;
        log_call(ctx, op);
    }
    if (info) *info = ctx->last_info;
    return RTDD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int rtdd_last_solve_info(rtdd_ctx *ctx, rtdd_solve_info *info) {
    if (!ctx || !info) return RTDD_ERR_INVALID;
    *info = ctx->last_info;
    return RTDD_OK;
}

int rtdd_scaled_mode_waves(rtdd_ctx *ctx, int *waves) {
    if (!ctx || !waves) return RTDD_ERR_INVALID;
    RTDD_TRY(rtdd_ctx_synchronize(ctx));
    DeviceGuard g(ctx->device);
    RTDD_HIP(ctx, hipMemcpy(waves, ctx->sync_words + kSyncScaled, sizeof(int), hipMemcpyDeviceToHost));      // (persist_sync.hpp: the waves count themselves)
    return RTDD_OK;
}

int rtdd_multigrid_level(rtdd_ctx *ctx, int level, int which, float *host, int *rows, int *cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, rows && cols, "null size pointers");
    DeviceGuard g(ctx->device);
    const int rc = mg_download(ctx, level, which, host, rows, cols);
    if (rc == RTDD_ERR_INVALID) return fail(ctx, rc, "no multigrid hierarchy, or level/plane out of range");
    return rc;
}

int rtdd_matrix_free_solver(rtdd_ctx *ctx, float *depth, size_t depthPitch, const uint8_t *scribble, size_t scribblePitch,
                            const uint8_t *gray, size_t grayPitch, int rows, int cols, float beta, int maxIterations,
                            float tolerance, int level) {
    (void)beta; (void)tolerance;                   // ignored by the reference too (src/GPUSolver.cu:274-275)
    if (!ctx) return RTDD_ERR_INVALID;
    if (maxIterations < 0) maxIterations = 0;      // the reference's loop simply does not run (:295)
    const rtdd_solve_params p{RTDD_METHOD_CHEBYSHEV_JACOBI, maxIterations, /*tolerance=*/0.0f, /*checkEvery=*/0, /*relaxation=*/0.0f};
    return solve_with(ctx, {depth, depthPitch, scribble, scribblePitch, gray, grayPitch, RTDD_GUIDE_GRAY, rows, cols, level, p, {}}, nullptr, nullptr);
}

int rtdd_index_to_weight(rtdd_ctx *ctx, const uint8_t *gray, size_t grayPitch, const float *depth, size_t depthPitch,
                         int32_t *index2, int level, int rows, int cols) {
    return rtdd_index_to_weight_guided(ctx, gray, grayPitch, RTDD_GUIDE_GRAY, depth, depthPitch, index2, level, rows, cols);
}

int rtdd_index_to_weight_guided(rtdd_ctx *ctx, const uint8_t *guide, size_t guidePitch, int guideKind, const float *depth, size_t depthPitch,
                                int32_t *index2, int level, int rows, int cols) {
    return rtdd_index_to_weight_regions(ctx, guide, guidePitch, guideKind, nullptr, 0, 0, depth, depthPitch, index2, level, rows, cols);
}

int rtdd_index_to_weight_regions(rtdd_ctx *ctx, const uint8_t *guide, size_t guidePitch, int guideKind, const uint8_t *regions, size_t regionsPitch,
                                 int regionFlags, const float *depth, size_t depthPitch, int32_t *index2, int level, int rows, int cols) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, (regionFlags & ~(RTDD_REGION_CUT | RTDD_REGION_SMOOTH)) == 0, "unknown region flag");
    REQUIRE(ctx, regions || regionFlags == 0, "region flags without a region image");
    REQUIRE(ctx, !regions || cols <= 0 || regionsPitch >= (size_t)cols, "region pitch smaller than a row");
    if (!regions) regionFlags = 0;
    const uint8_t *gray = guide;
    REQUIRE(ctx, guideKind == RTDD_GUIDE_GRAY || guideKind == RTDD_GUIDE_BGR, "unknown guide kind");
    const size_t grayPitch = guideKind == RTDD_GUIDE_BGR ? guidePitch / 3 : guidePitch;       // (compared with cols below: pitch >= 3 * cols)
    REQUIRE(ctx, gray && depth && index2, "null pointer");
    REQUIRE(ctx, rows > 0 && cols > 0 && grayPitch >= (size_t)cols && depthPitch >= (size_t)cols * 4, "bad size or pitch");
    REQUIRE(ctx, f32_image_aligned(depth, depthPitch), kF32AlignText);
    if (ctx->maxLevel < 0) return fail(ctx, RTDD_ERR_STATE, "rtdd_allocate has not been called (maxLevel unknown)");
    DeviceGuard g(ctx->device);
    // reads a depth image a logged, unconfirmed solve may not have written (its copy-back stores nothing after a time-out) and is not
    // logged itself: confirm or heal first.  Nothing logged: nothing to wait for.
    RTDD_TRY(settle_pending(ctx));
    return launch_index_to_weight(ctx, guide, guidePitch, depth, depthPitch, index2, level, rows, cols, guideKind, regions, regionsPitch, regionFlags);
}

// the packing rule of the pyramid's code planes (cascade.hip k_region_codes) on caller images: level `level` of a rows x cols pair
int rtdd_region_codes(rtdd_ctx *ctx, const uint8_t *edited, size_t editedPitch, const uint8_t *mask, size_t maskPitch, int rows, int cols,
                      int level, uint8_t *codes, size_t codesPitch) {
    if (!ctx) return RTDD_ERR_INVALID;
    REQUIRE(ctx, edited && mask && codes, "null image pointer");
    REQUIRE(ctx, rows >= 0 && cols >= 0 && rows <= 32768 && cols <= 32768, "size outside [0, 32768]");
    REQUIRE(ctx, level >= 0 && level < 16, "level outside [0, 15]");
    RegionLevels lv{};
    lv.n = 1; lv.shift[0] = level; lv.rows[0] = rows >> level; lv.cols[0] = cols >> level;       // the floor chain (rtdd_allocate's level sizes)
    if (lv.rows[0] == 0 || lv.cols[0] == 0) return RTDD_OK;
    REQUIRE(ctx, editedPitch >= (size_t)cols * 3 && maskPitch >= (size_t)cols && codesPitch >= (size_t)lv.cols[0], "pitch smaller than a row");
    lv.codes[0] = codes; lv.pitch[0] = codesPitch; lv.stride[0] = 0;
    DeviceGuard g(ctx->device);
    RTDD_TRY(pyramid_check_read(ctx, mask, edited));
    return launch_region_codes(ctx, edited, editedPitch, 0, mask, maskPitch, 0, lv, 1);
}

}  // extern "C"
#pragma GCC visibility pop
