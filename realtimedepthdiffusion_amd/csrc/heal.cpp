// heal.cpp -- the persistent kernels' host side: a launch's flag values, the log of calls no synchronising call has confirmed yet, and
// the replay of that log after a persistent launch gave up (persist_sync.hpp, include/rtdd.h RTDD_ERR_TIMEOUT).  Host code only.
#include "rtdd_internal.hpp"
#include "persist_sync.hpp"

namespace rtdd {

// The per-tile flags are never reset between launches: a persistent launch with `nblocks` blocks is handed the base value
// *flag_base = the context's running epoch, its workgroups publish and wait for flag_base + 1 .. flag_base + nblocks - 1, and the epoch
// advances past them.  Launches of one context are stream-ordered, so every flag a launch finds is below its base.  (Round 2 zeroed
// the 1024 flags with a hipMemsetAsync in front of every persistent launch: a ~5 us fill kernel per pyramid level and per solve.)
int prepare_persistent_launch(rtdd_ctx *ctx, int nblocks, int *flag_base) {
    if (ctx->flag_epoch > (1 << 30) - nblocks - 2) {                  // (once in ~10^7 solves) start over
        RTDD_HIP(ctx, hipMemsetAsync(ctx->sync_words + kSyncFlags, 0, (size_t)kSyncMaxTiles * kSyncFlagStride * sizeof(int), ctx->stream));
        ctx->flag_epoch = 0;
    }
    // (a launch's workgroups announce themselves with its base value: never the zero the flags start from)
    if (ctx->flag_epoch == 0) ctx->flag_epoch = 1;
    *flag_base = ctx->flag_epoch;
    ctx->flag_epoch += nblocks + 1;
    const int limit = ctx->opt.debug_poll_limit_us > 0 ? ctx->opt.debug_poll_limit_us * 100 : 0;        // 10 ns ticks
    // (RTDD_OPT_DEBUG_WITHHOLD_TILE is no control word: every persistent launch is handed ctx->opt.debug_withhold_tile as an argument,
    // the value at the time it is enqueued -- the order a stream-ordered write of the word gave; persist_sync.hpp exchange_wait_at)
    if (ctx->sync_limit != limit) {
        RTDD_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)(ctx->sync_words + kSyncLimit), limit, 1, ctx->stream));
        ctx->sync_limit = limit;
    }
    note_status_writer(ctx);
    return RTDD_OK;
}

// ---- self-healing ---------------------------------------------------------------------------------------------------------------
// The reference's GPUMatrixFreeSolver always leaves a valid depth map behind (src/GPUSolver.cu:311-314), and an unchanged main.cpp can
// neither set options nor upload its input again.  A persistent launch that is not fully co-resident (a shared GPU) gives up after its
// poll limit and sets the status word; from then on k_finish / k_pyrup_inject store nothing (persist_sync.hpp solve_is_dead), so every
// call made since keeps its INPUT, and the first of them has left its sequence number in sync_words[kSyncFailedSeq].  The next call that
// synchronises finds the word, switches persistence off for the rest of the context's life (one warning on stderr), runs the logged
// calls again from the failed one on, one launch per block of sweeps, and only then returns -- RTDD_OK, with the results the calls
// would have produced.  Status 2 (a wave waiting for a wave of its own workgroup: a protocol bug, not a scheduling accident) and a
// second failure during the replay are reported as RTDD_ERR_TIMEOUT as before.
static int replay(rtdd_ctx *ctx, const PendingOp &op, int failed_seq) {
    const Options now = ctx->opt;
    ctx->opt = op.opt;
    ctx->opt.persistent = 0;
    ctx->opt.debug_force_status = op.opt.debug_force_status == 3 ? 1 : 0;      // (3: the testing aid that makes the REPLAY fail as well)
    int rc = RTDD_OK;
    switch (op.kind) {
        case PendingOp::kSolve: rc = solve_with(ctx, op.solve, nullptr, nullptr); break;
        case PendingOp::kEstimate: rc = estimate_replay(ctx, op.estimate, failed_seq); break;
        case PendingOp::kEffect: rc = launch_effect(ctx, op.effect); break;
        default: rc = fail(ctx, RTDD_ERR_TIMEOUT, "unknown call in the pending log; the results since the last synchronisation are invalid");
    }
    ctx->opt = now;
    return rc;
}

// The one place a call enters the log: remembered until a copy-back kernel or a synchronising call has confirmed it.  Nothing is
// logged while a replay runs.  A solve or an estimate is logged whenever RTDD_OPT_TIMEOUT_HEAL is on; at capacity the log is cleared
// and pending_overflow set (a time-out among more calls than the log holds is reported, not healed).  A depth effect is logged only
// behind a log that is not empty, before and after the confirmed calls are dropped: should one of the unconfirmed solves in front of
// it turn out to have timed out, the effect ran on its INPUT and is run again behind the replayed solve (nothing unconfirmed: nothing
// to log); at capacity it is dropped and pending_overflow left alone.
bool log_call(rtdd_ctx *ctx, PendingOp &op) {
    const bool effect = op.kind == PendingOp::kEffect;
    if (ctx->healing || (effect ? ctx->pending.empty() : !ctx->opt.timeout_heal)) return false;
    prune_confirmed(ctx);
    if (effect && ctx->pending.empty()) return false;
    if (ctx->pending.size() >= kMaxPendingOps) {
        if (effect) return false;
        ctx->pending.clear(); ctx->pending_overflow = true;
    }
    op.id = ++ctx->op_counter;
    ctx->pending.push_back(op);
    return true;
}

// Sequence number of the kernel that publishes the LAST result of a logged call (0: the call publishes no solve).
static int last_seq(const PendingOp &op) {
    if (op.kind == PendingOp::kSolve) return op.seq;
    if (op.kind != PendingOp::kEstimate) return 0;
    int m = 0;
    for (int s : op.estimate.level_seq) if (s > m) m = s;
    return m;
}

// The copy-back kernels report, in page-locked memory, the sequence number of the latest solve whose result they published while the
// status word was clear (persist_sync.hpp solve_is_dead).  Every logged call up to and including that solve -- the effects queued in
// front of it too: they ran behind solves that had succeeded -- can never be asked for again, so it leaves the log here, without any
// synchronisation: the log holds the calls still in flight (plus the effects behind the last solve), not everything since the last
// rtdd_ctx_synchronize, and the caller's pointers are kept no longer than any asynchronous call keeps them.
void prune_confirmed(rtdd_ctx *ctx) {
    if (!ctx->confirm_host || ctx->pending.empty() || ctx->healing) return;
    const int confirmed = *(volatile int *)ctx->confirm_host;
    size_t n = 0;
    for (size_t i = 0; i < ctx->pending.size(); i++) {
        const int s = last_seq(ctx->pending[i]);
        if (s != 0 && s <= confirmed) n = i + 1;
    }
    if (n) ctx->pending.erase(ctx->pending.begin(), ctx->pending.begin() + n);
}

static bool op_holds(const PendingOp &op, int seq) {
    if (op.kind == PendingOp::kSolve) return op.seq == seq;
    if (op.kind != PendingOp::kEstimate) return false;
    for (int s : op.estimate.level_seq) if (s != 0 && s == seq) return true;
    return false;
}

static const char *kTimeoutText =
    "persistent sweep kernel: a workgroup timed out waiting for a neighbouring tile (its workgroups were not all "
                                  "co-resident: is the GPU shared?)";

// The stream has just been synchronised by the caller.  A blocked-sweep launch since the last check may have given up (persist_sync.hpp).
int check_persistent_status(rtdd_ctx *ctx, bool in_solve) {
    if (!ctx->persistent_used || !ctx->sync_words) {
        if (!ctx->healing) { ctx->pending.clear(); ctx->pending_overflow = false; }
        return RTDD_OK;
    }
    // The newest guarded copy-back kernel has reported its solve published with the status word clear, and nothing that could set a
    // control word was queued behind it: the words are clear (they are sticky, and that kernel ran behind every launch that could have
    // set them) -- no need to read them back.
    if (!ctx->healing && !ctx->status_writer_behind && ctx->publish_seq != 0 && ctx->confirm_host &&
        *(volatile int *)ctx->confirm_host == ctx->publish_seq) {
        ctx->persistent_used = false;
        ctx->pending.clear(); ctx->pending_overflow = false;
        return RTDD_OK;
    }
    int words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    RTDD_HIP(ctx, hipMemcpy(words, ctx->sync_words, sizeof(words), hipMemcpyDeviceToHost));
    ctx->persistent_used = false;
    const int status = words[kSyncStatus], failed_seq = words[kSyncFailedSeq];
    // a defocus kernel summed windows by hand: not a depth map -- bit 0: the tile kernel, the table path
    if (words[kSyncNonLocal] != 0) {
                                                   // from now on; bit 1: a banded table, one whole-image table from now on
        if (words[kSyncNonLocal] & 1) ctx->defocus_table_sticky = true;
        if (words[kSyncNonLocal] & 2) ctx->defocus_band_sticky = true;
        RTDD_HIP(ctx, hipMemset(ctx->sync_words + kSyncNonLocal, 0, sizeof(int)));
    }
    if (status == 0) { if (!ctx->healing) { ctx->pending.clear(); ctx->pending_overflow = false; } return RTDD_OK; }
    RTDD_HIP(ctx, hipMemset(ctx->sync_words + kSyncStatus, 0, sizeof(int)));
    RTDD_HIP(ctx, hipMemset(ctx->sync_words + kSyncFailedSeq, 0, sizeof(int)));
    if (status != 1) {
        ctx->pending.clear(); ctx->pending_overflow = false;
        return fail(ctx, RTDD_ERR_TIMEOUT,
            "blocked sweep kernel: a wave timed out waiting for a neighbouring wave of its own workgroup (internal error); "
                                           "the results since the last synchronisation are invalid");
    }
    // Persistence off, and suspended: rearm_after solves after the first heal, twice as many after every further one, for good after
    // kMaxRearms heals (an unchanged main.cpp on the drop-in shim can set no option: one scheduling accident on a shared GPU must not
    // cost it the persistent kernel until exit, and a GPU that stays shared must not cost it a 200 ms stall every few frames).
    if (!ctx->healing) {                            // (a second time-out while the calls are being run again is part of the same event)
        ctx->opt.persistent = 0;
        ctx->heals++;
        if (ctx->heals > kMaxRearms || ctx->opt.rearm_after <= 0) ctx->persist_suspend = -1;
        else {
            const long long n = (long long)ctx->opt.rearm_after << (ctx->heals - 1);
            ctx->persist_suspend = n > (1 << 30) ? (1 << 30) : (int)n;
        }
    }
    if (ctx->healing || ctx->pending_overflow || !ctx->opt.timeout_heal) {
        std::string msg = kTimeoutText;
        msg += ctx->healing ? "; it happened again while the calls were being run again without persistence"
             : !ctx->opt.timeout_heal ? "; RTDD_OPT_TIMEOUT_HEAL is 0, so nothing was run again"
                 : "; too many calls were queued without a synchronisation to run them again";
        msg += "; the results since the last synchronisation are invalid";
        ctx->pending.clear(); ctx->pending_overflow = false;
        return fail(ctx, RTDD_ERR_TIMEOUT, msg.c_str());
    }
    // heal: the logged calls again from the first failed one
    if (!ctx->heal_warned) {
        ctx->heal_warned = true;
        std::fprintf(stderr,
                     "rtdd: %s; running the affected calls again one launch per block of sweeps -- persistent launches are suspended "
                     "for this context's next %d solves (twice as long after every further time-out, for good after %d)\n",
                     kTimeoutText, ctx->persist_suspend, kMaxRearms);
    }
    std::vector<PendingOp> ops;
    ops.swap(ctx->pending);
    size_t first = ops.size();                      // failed_seq == 0: every logged call had published its result before the word was set
    if (failed_seq != 0) {
        for (size_t i = 0; i < ops.size(); i++) if (op_holds(ops[i], failed_seq)) { first = i; break; }
        if (first == ops.size()) return fail(ctx, RTDD_ERR_TIMEOUT,
            "persistent sweep kernel timed out and the failed call is not among the logged ones; the results since the last "
            "synchronisation are invalid");
    }
    ctx->healing = true;
    ctx->heal_rebuilt = false;
    int rc = RTDD_OK;
    for (size_t i = first; i < ops.size() && rc == RTDD_OK; i++) rc = replay(ctx, ops[i], i == first ? failed_seq : 0);
    if (rc == RTDD_OK) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, RTDD_ERR_HIP, "hipStreamSynchronize (replay)", e);
        else { note_status_writer(ctx); rc = check_persistent_status(ctx); }
    }
    ctx->healing = false;
    if (rc != RTDD_OK) return rc;
    return in_solve ? kRestartSolve : RTDD_OK;
}

// Calls that change what a logged solve / estimate would run on (the level planes, the weight table, the pyramid's images) first
// settle the log: synchronise and look at the status word while the state the logged calls were made against still exists.
int settle_pending(rtdd_ctx *ctx) {
    if (ctx->pending.empty() || ctx->healing) return RTDD_OK;
    RTDD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return check_persistent_status(ctx);
}

}  // namespace rtdd
