// persist_sync.hpp -- the inter-workgroup hand-off of the persistent kernels (sweep_blocked.hip, rbgs_blocked.hip), device side,
// and the host helpers around it (heal.cpp).
//
// Control words (rtdd_ctx::sync_words, device memory, one set per context):
//   [kSyncStatus]    0 = fine; 1 = a workgroup gave up waiting for a neighbouring TILE (the launch was not fully co-resident:
//                    GPU shared with another stream or process); 2 = a wave gave up waiting for a neighbouring WAVE of its own
//                    workgroup (cannot happen -- every wave of a workgroup is resident -- so: a protocol bug).  Sticky until the
//                    host reads it (rtdd_ctx_synchronize and every other call that synchronises anyway) and returns
//                    RTDD_ERR_TIMEOUT.  Once it is set every workgroup that sees it stops exchanging and returns, and every
//                    later persistent launch returns at once, so a failed estimate drains in microseconds instead of spinning
//                    through its remaining exchanges.
//   [kSyncWithhold]  reserved, never written or read (it held RTDD_OPT_DEBUG_WITHHOLD_TILE until the persistent kernels were handed that
//                    value as an argument -- exchange_wait_at's `withhold`; the index stays so that the layout does not move).
//   [kSyncLimit]     poll limit in 10 ns ticks of s_memrealtime (0 = kDefaultPollLimit).
//   [kSyncFailedSeq] sequence number of the first solve whose copy-back kernel (k_finish / k_pyrup_inject) found the status word set and
//                    therefore stored nothing: the host re-runs the pending calls from that one on (heal.cpp check_persistent_status).  0 = none.
//   [kSyncConfirmPtr] (two ints, an address) where the copy-back kernels report the sequence number of a solve whose result they DID publish:
//                    a word in page-locked host memory, so that the host can drop confirmed calls from its log without synchronising
//                    (heal.cpp prune_confirmed).  Written by one lane, only while the status word is clear.
//   [kSyncWild]      sequence number of the most recent solve whose k_prepare met a depth that is not finite or is 2^100 or larger in
//                    magnitude (solver_kernels.hip; a plain vector store, made only when such a value is found).  The register-blocked
//                    sweep kernels compare it with their own solve's number and, when equal, run the variant with the full IEEE divide
//                    and explicit absent neighbours (sweep_common.hpp div_tail).  Never cleared: sequence numbers do not repeat.
//   [kSyncLarge]     sequence number of the most recent solve whose k_prepare met a depth of 2^32 or more in magnitude (or not finite: every
//                    wild depth is large too).  Raised where kSyncWild is raised and in the same way.  The persistent sweep compares it with
//                    its solve's number: when equal, no wave of the launch enters SCALED MODE (sweep_common.hpp div_scaled4 / div_scaled, whose numerator
//                    times 2^64 must not overflow).  The word behind kSyncWild, so that the kernel reads both with one 8-byte load.
//   [kSyncScaled]    how many waves have entered scaled mode over the life of the context.  Waves that enter at the start of a launch
//                    (sweep_blocked.hip kFromStart: every eligible wave of a 1080p launch, 4032 of them) count themselves in LDS, and one
//                    lane per WORKGROUP adds their number; a wave that enters on demand, at a block boundary, adds 1 from one lane (once
//                    per wave and launch, on the cold path).  Read back by rtdd_scaled_mode_waves, for the tests: nothing in the product
//                    depends on it.
//   [kSyncFlags ..]  one block counter per tile.  Monotonic over the life of the context: launch L's workgroups publish base_L + block
//                    number, base_L handed in by the host (heal.cpp prepare_persistent_launch), so nothing is zeroed between launches.
#pragma once
#include <hip/hip_runtime.h>

namespace rtdd {

// kSyncFlagStride: ints between the flags of consecutive tiles.  64 = one flag per 256 bytes (its own line, and neighbouring tiles on different memory channels): a tile's flag is stored once and polled
// by up to 8 neighbours, all through memory (sc1); packed 32 to a line (round 2) every store and poll of 32 tiles met on one line: 1080p 1.17 -> 1.24 Tpx-it/s with one line each, +1.5 % more at 256 bytes.
constexpr int kSyncStatus = 0, kSyncWithhold = 1, kSyncLimit = 2, kSyncNonLocal = 3 /* k_defocus_tile met windows beyond its region (effect_kernels.hip) */, kSyncFailedSeq = 4,
              kSyncConfirmPtr = 6 /* two ints: the device address of the context's page-locked `confirmed sequence number` word */, kSyncWild = 8, kSyncLarge = 9 /* = kSyncWild + 1: one 8-byte load */, kSyncScaled = 10, kSyncFlags = 32, kSyncMaxTiles = 1024, kSyncFlagStride = 64;
constexpr int kSyncWords = kSyncFlags + kSyncMaxTiles * kSyncFlagStride;              // size of sync_words in ints
constexpr unsigned long long kDefaultPollLimit = 20000000ull;      // 200 ms: legitimate waits are microseconds
// Round 6: the FIRST thing a persistent workgroup does is announce itself (its flag := the launch's base value) and wait for its
// neighbours' announcements -- while its tile loads are in flight -- with THIS bound: on a GPU shared with other work a launch whose
// workgroups are not all resident is found out here, before any sweep, in 1.5 ms instead of 200 (profiles/r05_shared_gpu.txt: a
// 200 ms stall per time-out in a 1 ms frame loop).  A resident launch's workgroups all start within tens of microseconds.  The
// exchanges behind the first keep the long bound: once every workgroup has been seen running, a long wait is no scheduling accident.
constexpr unsigned long long kArrivalPollLimit = 150000ull;        // 1.5 ms

// A depth of this magnitude or more (or a NaN) makes k_prepare raise kSyncWild.  An iterate that starts below it cannot reach an
// overflowing numerator: the mean r is clamped to [0, 255], so x_{k+1} = 0.01 omega x_k + (1 - omega) x_{k-1} + 0.99 omega r is a
// bounded forcing on a recurrence whose characteristic roots have modulus sqrt(omega - 1) < 1 for the schedule's omega in [1, 2) --
// the iterates stay within a small multiple of the start, while a sum of four of them (weights <= 1) overflows only from 2^125 on,
// and the 3-operation divide's q0 = n * y is within an ulp of a weighted mean, no larger than the largest of them.  Red-black: the
// update is clamped to [0, 255] outright.  (tests/wild_depth.py: `magnitudes` runs just below the threshold, `huge` above it.)
constexpr float kWildDepth = 0x1p100f;
// A depth of this magnitude or more (or a NaN) makes k_prepare raise kSyncLarge as well.  By the same argument an iterate that starts below
// it stays within a small multiple of 2^32, and a sum of four of them (weights <= 1) below 2^64 with about 2^30 to spare: the numerator
// div_scaled4 and div_scaled multiply by 2^64 stays finite.  Depth maps in [0, 255] never raise the word.
constexpr float kLargeDepth = 0x1p32f;

#ifdef __HIPCC__
// true when depth value d must send its solve to the sweep kernels' full-divide variant (NaN compares false)
__device__ __forceinline__ bool depth_is_wild(float d) { return !(__builtin_fabsf(d) < kWildDepth); }
// The word a sweep kernel compares with its solve's number (k_prepare ran in an earlier launch of the same stream).  Read at the TOP
// of the kernel, next to the tile loads: read where it is used, behind the setup, the load sits alone on every launch's critical
// path while the chip's tile loads are in flight (4K, 125 launches per solve: 5 % slower; EXPERIMENTS.md).
__device__ __forceinline__ int load_wild_word(const int *sync_words) { return sync_words[kSyncWild]; }
__device__ __forceinline__ bool depth_is_large(float d) { return !(__builtin_fabsf(d) < kLargeDepth); }
// What every prepare body does with a depth it has read (plain vector stores, made only when such a value is found).
__device__ __forceinline__ void raise_depth_words(int *sync_words, bool wild, bool large, int seq) {
    if (wild) sync_words[kSyncWild] = seq;
    if (large) sync_words[kSyncLarge] = seq;
}
// kSyncWild and kSyncLarge in one load (.x, .y): the persistent sweep's, at the same place as load_wild_word and for the same reason.
static_assert(kSyncLarge == kSyncWild + 1 && kSyncWild % 2 == 0, "the two words are read as one aligned pair");
__device__ __forceinline__ int2 load_wild_and_large_words(const int *sync_words) { return *(const int2 *)(sync_words + kSyncWild); }
// The kernels that publish a solve's result into the caller's buffers call this first (every thread; `first` = one thread of the
// grid): true = a sweep launch in front of them gave up, store nothing.  The reference's solver always leaves a valid depth map
// (src/GPUSolver.cu:311-314); here a failed solve leaves its INPUT in place so that the host can run it again.
__device__ __forceinline__ bool solve_is_dead(int *sync_words, int seq, bool first) {
    if (!sync_words) return false;
    if (__hip_atomic_load(&sync_words[kSyncStatus], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        if (first && seq != 0) {                   // this solve's result is being published: tell the host (one lane, one posted write)
            int *confirm = *(int *const *)(sync_words + kSyncConfirmPtr);
            if (confirm) __hip_atomic_store(confirm, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return false;
    }
    if (first && __hip_atomic_load(&sync_words[kSyncFailedSeq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_store(&sync_words[kSyncFailedSeq], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// The flag a thread polls, as a byte offset from sync_words: lane i (of 9, i != 4) of wave 0 polls neighbour (i%3-1, i/3-1); -1 = this
// thread polls nothing.  It depends on the thread and the tile only, so a kernel that exchanges many times works it out once
// (sweep_blocked.hip keeps it in its exchange record) and hands it to exchange_wait_at().
__device__ __forceinline__ int exchange_poll_offset(int tid, int bx, int by, int gx, int gy, int tile_base) {
    const int pw = tid >> 6, pl = tid & 63;
    if (pw != 0 || pl >= 9 || pl == 4) return -1;
    const int nx = bx + pl % 3 - 1, ny = by + pl / 3 - 1;
    if (nx < 0 || ny < 0 || nx >= gx || ny >= gy) return -1;
    return (kSyncFlags + (tile_base + ny * gx + nx) * kSyncFlagStride) * (int)sizeof(int);      // (< 2^31: kSyncWords ints)
}

// A flag read as the relaxed agent-scope atomic load it is (global_load_dword sc1 and its wait), written out so that the address stays
// scalar base + 32-bit lane offset inside the polling loop (left to the compiler the loop keeps a 64-bit sum per lane).
// The s_nop 4 in front: the compiler pads no hazard whose consumer is inside an asm string, and where it has spilled `base` to a VGPR lane
// it restores it with v_readlane_b32 directly in front of the statement -- a VALU write of an SGPR that a VMEM instruction reads needs 5
// wait states, or the load goes to whatever the pair held before (k_sweep_blocked<32, 512, 6, true, true> faulted that way; EXPERIMENTS.md
// "Tile 3").  The same opening is in every statement of sweep_common.hpp that addresses through a scalar base; tests/test_isa_narrowed_exec.py
// checks the wait states on the built objects.  Five cycles per poll, next to an s_sleep.
__device__ __forceinline__ int load_flag_at(const int *base, unsigned off) {
    int v;
    asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(off), "s"(base) : "memory");
    return v;
}

// Called by EVERY thread of the workgroup after its payload stores are drained (s_waitcnt vmcnt(0)) and a __syncthreads().
// Publishes this tile's counter, waits for the up-to-8 neighbouring tiles' counters, makes their payload visible (one agent
// acquire by wave 0) and ends with a __syncthreads().  Returns true when the launch is dead (see kSyncStatus): the caller
// leaves.  `dead_lds` is a __shared__ int, zero at kernel start.
// Protocol (cdna_hip_programming.md Guideline 16, R1): write-through (sc1) payload stores; EVERY storing wave drains vmcnt;
// workgroup barrier; ONE lane stores the flag (agent-scope atomic); 8 lanes poll the neighbours' flags relaxed with s_sleep;
// ONE agent acquire; barrier; plain vector loads.
// exchange_wait_at() is exchange_wait() with the polled flag's place worked out by the caller (exchange_poll_offset): the flag is addressed as the
// scalar base sync_words plus that 32-bit offset, so an exchange forms no 64-bit address per lane.
// `withhold`: the testing aid RTDD_OPT_DEBUG_WITHHOLD_TILE -- tile number + 1 whose flag is never published (in a batch: every image's
// tile of that number), 0 = off -- to make the time-out path testable.  A KERNEL ARGUMENT, the option's value when the launch was
// enqueued: as a control word read here it was a trip to L2 and a vmcnt wait between the barrier and the flag store of every exchange,
// exactly where every tile of the grid is waiting for its neighbours' flags (tests/test_isa_exchange_chain.py).
template <bool ACQUIRE = true, bool ARRIVAL = false>
__device__ __forceinline__ bool exchange_wait_at(int *sync_words, int *dead_lds, int tid, int tile_id, int poll_off, int value, int withhold, int tile_base = 0) {
    int *flags = sync_words + kSyncFlags + tile_base * kSyncFlagStride;      // (tile_base: a batched launch gives every image's tiles flags of their own)
    if (tid == 0 && withhold != tile_id + 1) {
        // The flag's address is scalar; the store still wants a vector offset, 0.  It is made HERE (no instruction but the v_mov_b32 of
        // the constant): left to the register allocator the 1024-thread tile of four rows per thread, which sits at its cap of 128
        // registers, reloaded a spilled tuple of zeros from scratch for it and waited for that load in front of the flag store.
        unsigned zero = 0;
        asm volatile("" : "+v"(zero));
        __hip_atomic_store((int *)((char *)&flags[tile_id * kSyncFlagStride] + zero), value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // A poll is a round trip to memory (the flag was stored sc1: it is in no L2).  (Several polling waves, each started a fraction of a
    // trip after the one before and the first to see all its neighbours telling the others through LDS, measured no faster: EXPERIMENTS.md.)
    if (poll_off >= 0) {
        unsigned long long t0 = 0, limit = 0;
        unsigned spins = 0;
        while (load_flag_at(sync_words, (unsigned)poll_off) - value < 0) {
            __builtin_amdgcn_s_sleep(4);
            if ((++spins & 63u) == 0) {                              // every 64 polls (tens of microseconds): clock and status word
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                if (t0 == 0) {
                    t0 = now;
                    const int l = __hip_atomic_load(&sync_words[kSyncLimit], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    limit = l > 0 ? (unsigned long long)l : kDefaultPollLimit;
                    if (ARRIVAL && limit > kArrivalPollLimit) limit = kArrivalPollLimit;
                }
                const bool failed = __hip_atomic_load(&sync_words[kSyncStatus], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (failed || now - t0 > limit) {
                    if (!failed) __hip_atomic_store(&sync_words[kSyncStatus], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(dead_lds, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
            }
        }
    }
    // ACQUIRE = false: the caller reads the handed-off bytes with 16-byte sc1 loads only (MI355X_MICROARCH.md, "Valid forms": the
    // polling wave after its poll has matched, the other waves after the barrier below)
    if (ACQUIRE && tid < 64) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    if (!ACQUIRE && tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the polls themselves have returned
    __syncthreads();
    return __hip_atomic_load(dead_lds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
}

template <bool ACQUIRE = true, bool ARRIVAL = false>
__device__ __forceinline__ bool exchange_wait(int *sync_words, int *dead_lds, int tid, int tile_id, int bx, int by, int gx, int gy, int value, int withhold, int tile_base = 0) {
    return exchange_wait_at<ACQUIRE, ARRIVAL>(sync_words, dead_lds, tid, tile_id, exchange_poll_offset(tid, bx, by, gx, gy, tile_base), value, withhold, tile_base);
}

#endif

}  // namespace rtdd
