// sweep_tile_sweeps.inc -- included INSIDE the body of k_sweep_blocked (sweep_blocked.hip): the per-wave publish / await of edge rows
// through LDS and ONE sweep of the register-resident tile, as lambdas over the tile's registers.
// Expects in scope: PERSIST (constexpr bool), tiny_state and kMetTiny (int: the bit a fast sweep of a persistent wave sets when it takes its tiny branch; kFromStart (constexpr bool): a wave in scaled mode holds d * 2^64 / y * 2^-64 in cnt[] / rcp[] and divides by div_scaled4), CONTRACT, G, LX, edge[], published[], dead_s, sync_words, omegas, gamma, tid, lx, tr, ntr,
// bx, by, gx and the tile registers of sweep_tile_setup.inc.
    constexpr uint32_t kTinyT = 2u * 0x0D800000u - 1u;          // bits(2^-100) = 27 << 23
    const int prev4 = (((int)threadIdx.x + 63) & 63) * 4;       // horizontal neighbours across lanes by ds_bpermute_b32, issued a group ahead (sweep_common.hpp: why not DPP)
    const int wv = tid >> 6, nwv = (int)blockDim.x >> 6;
    const int tile_id_tl = by * gx + bx; (void)tile_id_tl;
    auto publish = [&](const f4r &top, const f4r &bottom, int sweep_no, int buf) {      // rows that sweep `sweep_no` of the neighbours reads
        // (buf = sweep_no & 1, passed separately so that it is a compile-time constant in the unrolled sweep pair: every block
        // starts at an even sweep)
        *(f4r *)&edge[buf][tr][0][lx] = top;
        if (G > 1) *(f4r *)&edge[buf][tr][1][lx] = bottom;       // (G == 1: one row is both; the readers below take slot 0 -- half the LDS writes of the coarse levels' tile)
        if (!PERSIST) {
            // The LDS serves one wave's accesses in order, so the counter store needs no drained lgkmcnt in front of it: compiler
            // barriers only (+1 % at 4K, -1 % on the estimate).  The persistent instantiation keeps the release store: there the
            // same change costs 4 % (it moves the 128-register allocation of the 1024-thread tile).
            asm volatile("" ::: "memory");
            __hip_atomic_store(&published[wv], sweep_no + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            asm volatile("" ::: "memory");
        } else {
            __hip_atomic_store(&published[wv], sweep_no + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    unsigned lds_spins = 0;
    bool gone = false;                       // the launch is dead (dead_s is set): this wave stops waiting for its neighbours; the whole
                                             // workgroup leaves together at the next exchange (exchange_wait returns true for everyone)
    auto await = [&](int sweep_no) {
        if (gone) return;
        // both neighbours' counters in one LDS access: lane 0 reads the wave above, every other lane the wave below
        const int idx = (tid & 63) == 0 ? (wv > 0 ? wv - 1 : wv) : (wv < nwv - 1 ? wv + 1 : wv);
        // one compare + one scalar branch on the lane mask (two v_readlane + s_min + s_cmp before: the poll sits on every wave's
        // critical path -- +3 % at 1080p, -6 % on the coarse-to-fine estimate)
        auto there = [&]() { return __builtin_amdgcn_ballot_w64(__hip_atomic_load(&published[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < sweep_no + 1) == 0; };
        if (__builtin_expect(!there(), 0)) {                              // the first read usually succeeds: the waiting loop stays out of the straight
                                                                          // path (as one loop the structurizer put six scalar ops and two taken branches
                                                                          // behind every successful read: +2 % at 1080p and 4K)
            for (;;) {
                __builtin_amdgcn_s_sleep(1);
                if (there()) break;
                if ((++lds_spins & 1023u) == 0) {                        // a neighbouring wave that has LEFT (dead launch) never publishes again
                    if (__hip_atomic_load(&dead_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0) { gone = true; break; }
                    if (lds_spins > (1u << 22)) {                        // seconds: every wave of a workgroup is resident, so this is a bug -- say so, never hang
                        __hip_atomic_store(&sync_words[kSyncStatus], 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(&dead_s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        gone = true; break;
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    auto sweep = [&](f4r (&cur)[G], f4r (&oth)[G], int s, auto fast, bool last_of_block, auto parity) {
        // `fast`: std::false_type = the IEEE divide and explicit absent neighbours, std::true_type = the 3-operation divide with the tiny test
        // behind it, DivScaled = every quotient by div_scaled4 (the from-start tile, whose cnt[] / rcp[] hold d * 2^64 / y * 2^-64) or div_scaled (the on-demand tiles) -- a persistent wave in scaled mode, sweep_blocked.hip: no test, no branch
        constexpr int MODE = (int)decltype(fast)::value;
        constexpr bool FAST = MODE == 1, SCALED = MODE == 2, IEEE = MODE == 0;
        constexpr int buf = decltype(parity)::value;         // = s & 1
        RTDD_TL(0, s);
        // The first / last thread row of the tile has no row above / below in LDS: it reads its OWN published row instead (any
        // finite value will do -- the weight towards it is 0 at the image border, and elsewhere that row is discarded halo), which
        // keeps the two loads unconditional: no lane masks, no zero-filling moves.  (Not finite: the full-divide variant, below.)
        float xl0[G], xr3[G];                    // filled per group (each costs a register until its row is done)
        // the values a row needs from the neighbouring lanes: the previous lane's wr[g][3] * cur[g][3] (the whole left term of pixel 0)
        // and the next lane's cur[g][0].  They depend on x_k only, so they are requested before the rows that use them are started.
        // The full-divide variant also runs on inputs with infinities and NaNs (persist_sync.hpp kSyncWild), where 0 * x is no longer 0:
        // what a tile row's first lane receives from the lane before it and its last lane from the lane behind it, and (below) the rows
        // the first / last thread row reads in place of a row above / below, are 0 there -- each is an absent neighbour at the image
        // border, which the reference skips, or discarded halo.
        auto shifts = [&](int g) {
            xl0[g] = lds_from_prev(prev4, wr[g][3] * cur[g][3]); xr3[g] = lds_from_next(prev4, cur[g][0]);
            if (IEEE) { xl0[g] = lx == 0 ? 0.0f : xl0[g]; xr3[g] = lx == LX - 1 ? 0.0f : xr3[g]; }
        };
        shifts(0); if (G > 1) shifts(G - 1);                 // in flight during the wait for the neighbouring waves' rows
        await(s);
        float4 up4 = edge[buf][tr > 0 ? tr - 1 : 0][G > 1 && tr > 0 ? 1 : 0][lx];
        float4 dn4 = edge[buf][tr < ntr - 1 ? tr + 1 : tr][G == 1 || tr < ntr - 1 ? 0 : 1][lx];
        if (IEEE) { if (tr == 0) up4 = make_float4(0, 0, 0, 0); if (tr == ntr - 1) dn4 = make_float4(0, 0, 0, 0); }
        const float up[4] = {up4.x, up4.y, up4.z, up4.w}, dn[4] = {dn4.x, dn4.y, dn4.z, dn4.w};
        RTDD_TL_ROWS_IN_HAND(s);
        // omega and gamma in VGPRs: an fma with an SGPR operand issues at 4.3 cycles per wave-instruction, with three VGPRs at 3.1
        // (profiles/r05_excp_probe.txt); one v_mov per wave and sweep -- of omega only in the from-start tile's scaled sweeps, which take gamma
        // from the register the wave made in front of the block loop (sweep_blocked.hip DivScaledFromStart)
        float omega_v = omegas[s], gamma_v = gamma;
        if constexpr (SCALED && kFromStart) { gamma_v = fast.gamma; asm volatile("" : "+v"(omega_v)); }
        else asm volatile("" : "+v"(omega_v), "+v"(gamma_v));
        // weighted sum of pixel (g, i): solveDiffusion, src/GPUSolver.cu:73-106, absent neighbours carried as (w = 0, x = 0)
        auto wsum = [&](int g, int i) {
            const float xl = i == 0 ? xl0[g] : cur[g][i - 1];
            const float xr = i == 3 ? xr3[g] : cur[g][i + 1];
            const float xu = g == 0 ? up[i] : cur[g - 1][i];
            const float xd = g == G - 1 ? dn[i] : cur[g + 1][i];
            const float wu = g == 0 ? wu0[i] : wd[g - 1][i];
            // xl0[g] holds the previous lane's wr[g][3] * cur[g][3]; RN(wl * xl) + 0 is what fma(wl, xl, 0) and 0 + wl * xl both give
            // (the scaled pair of the from-start tile starts the chain AT the left term, without the `0 +`: a sum that is -0 in place of +0 is
            // all that can come of it, and div_scaled4 answers +0 to both -- sweep_common.hpp)
            float sum;
            if constexpr (SCALED && kFromStart) sum = i == 0 ? xl0[g] : (CONTRACT ? __builtin_fmaf(wr[g][i - 1], xl, 0.0f) : wr[g][i - 1] * xl);
            else sum = i == 0 ? 0.0f + xl0[g] : (CONTRACT ? __builtin_fmaf(wr[g][i - 1], xl, 0.0f) : 0.0f + wr[g][i - 1] * xl);
            sum = CONTRACT ? __builtin_fmaf(wr[g][i], xr, sum) : sum + wr[g][i] * xr;
            sum = CONTRACT ? __builtin_fmaf(wu, xu, sum) : sum + wu * xu;
            sum = CONTRACT ? __builtin_fmaf(wd[g][i], xd, sum) : sum + wd[g][i] * xd;
            return sum;
        };
        // rows g of the group selected by `pick`: quotients, the tiny test, updates
        auto group = [&](auto pick) {
            float q[G][4], sums[G][4];
            uint32_t tmin = 0xFFFFFFFFu;
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (!pick(g)) continue;
                uint32_t t[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if constexpr (SCALED && kFromStart) { q[g][i] = div_scaled4(wsum(g, i), cnt[g][i], rcp[g][i]); continue; }      // (cnt / rcp hold D / ys)
                    else if constexpr (SCALED) { q[g][i] = div_scaled(wsum(g, i), cnt[g][i], rcp[g][i]); continue; }
                    const float sum = sums[g][i] = wsum(g, i);
                    if (FAST) { q[g][i] = div_tail(sum, cnt[g][i], rcp[g][i]); t[i] = (__float_as_uint(sum) << 1) + 0xFFFFFFFFu; }
                    else q[g][i] = sum / cnt[g][i];
                }
                if (FAST) { tmin = min(min(tmin, t[0]), t[1]); tmin = min(min(tmin, t[2]), t[3]); }
            }
            if (FAST && __builtin_expect(__builtin_amdgcn_ballot_w64(tmin < kTinyT) != 0, 0)) {      // wave-uniform; rare on synthetic images, not on photographs
                // The tiny lanes take the scaled quotient (sweep_common.hpp div_tiny: ten plain operations, rounded once, against the divide's
                // 11 with its v_rcp_f32 and v_div_*); every other lane gets the quotient it had again (its scale is 1).
                // The persistent tiles have the registers to keep a row's four sums up to here; the launch-per-block tiles sit at their cap
                // of 128 and form each sum again where it is used, as the redo always did.
                auto sum_of = [&](int g, int i) { return PERSIST ? sums[g][i] : wsum(g, i); };
                if constexpr (PERSIST) tiny_state |= kMetTiny;      // (wave-uniform, a scalar: the wave may enter scaled mode at the next block boundary)
#pragma unroll
                for (int g = 0; g < G; g++) {
                    if (!pick(g)) continue;
#pragma unroll
                    for (int i = 0; i < 4; i++) q[g][i] = div_tiny(sum_of(g, i), cnt[g][i], rcp[g][i]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (!pick(g)) continue;
                float t[4], o[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float r = __builtin_amdgcn_fmed3f(q[g][i], 0.0f, 255.0f);        // :104; cnt == 0 was replaced by 1 (sum is 0 there): r = 0 (:103)
                    const float x = cur[g][i];
                    o[i] = oth[g][i];
                    // src/GPUSolver.cu:259, all but its last operation (the from-start tile's scaled pair: the same fma as ONE three-address
                    // instruction in every row -- sweep_common.hpp fma_vvv)
                    if constexpr (SCALED && kFromStart && CONTRACT) t[i] = fma_vvv(gamma_v, r - x, x) - o[i];
                    else t[i] = (CONTRACT ? __builtin_fmaf(gamma_v, r - x, x) : gamma_v * (r - x) + x) - o[i];
                    if (!CONTRACT) t[i] = omega_v * t[i];
                }
                // x_{k+1} = fma(omega, t, x_{k-1}) replaces x_{k-1} on the free pixels; a Dirichlet pixel's register already holds its value
                if (CONTRACT) masked_fmac4(o[0], o[1], o[2], o[3], omega_v, t[0], t[1], t[2], t[3], free_mask[g][0], free_mask[g][1], free_mask[g][2], free_mask[g][3]);
                else masked_add4(o[0], o[1], o[2], o[3], t[0], t[1], t[2], t[3], free_mask[g][0], free_mask[g][1], free_mask[g][2], free_mask[g][3]);
#pragma unroll
                for (int i = 0; i < 4; i++) oth[g][i] = o[i];
            }
        };
        // The rows the neighbouring waves wait for (first and last) are computed at a raised wave priority, the interior rows at the normal
        // one: the VALU arbiter then serves the waves that are on some other wave's critical path first (1080p 1.25 -> 1.29 Tpx-it/s, 4K
        // +1.5 %; priority 3, raising it from the top of the sweep, or keeping it raised for the younger half of the waves: no better /
        // worse -- EXPERIMENTS.md).
        __builtin_amdgcn_s_setprio(1);
        group([](int g) { return g == 0; });
#pragma unroll
        for (int gi = 1; gi < G - 1; gi++) shifts(gi);       // the interior rows' shifts: in flight while the last row is computed
        if (G > 1) group([](int g) { return g == G - 1; });
        if (!last_of_block) publish(oth[0], oth[G - 1], s + 1, buf ^ 1);
        __builtin_amdgcn_s_setprio(0);
        RTDD_TL(2, s);
#pragma unroll
        for (int gi = 1; gi < G - 1; gi++) group([gi](int g) { return g == gi; });
        // (no instruction: the row just written passes through one statement as FOUR CONSECUTIVE registers.  The one-row persistent tiles
        // otherwise keep x_{k-1} in one place during the sweeps and in another at the halo exchange, whose 16-byte loads need the row
        // consecutive, and move it there and back at every exchange -- tests/test_isa_exchange.py)
        if constexpr (PERSIST && G == 1) asm volatile("" : "+v"(oth[0]));
        if constexpr (PERSIST && G == 2 && SCALED) asm volatile("" : "+v"(oth[0]), "+v"(oth[1]));      // (the two-row tiles in scaled mode: sweep_blocked.hip, between the loops)
        RTDD_TL(3, s);
    };

