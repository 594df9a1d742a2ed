// sweep_common.hpp -- device helpers of the register-resident sweep kernels (sweep_blocked.hip): DPP lane
// shifts, the write-through stores / sc1 loads of the inter-workgroup hand-off, the 3-operation divide and the rounded reciprocal.
#pragma once
#include <hip/hip_runtime.h>

namespace rtdd {

// bound_ctrl: the lane without a source (lane 0 / lane 63) reads 0 -- its value is never used (the weight towards it is 0
// or the lane lies in the discarded halo) -- and the builtin needs no copy of `v` for the unwritten lane.
__device__ __forceinline__ float lane_from_prev(float v) {   // lane l <- lane l-1  (DPP wave_shr:1)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_from_next(float v) {   // lane l <- lane l+1  (DPP wave_shl:1)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xF, 0xF, true));
}

// The same two shifts through the LDS crossbar (ds_bpermute_b32: no LDS memory, no VALU slot), issued a group of rows ahead so that
// their latency hides behind the wait for the neighbouring waves' rows: k_sweep_blocked measured +3-5 % with them (1080p 1.17 -> 1.21
// Tpx-it/s, one tile alone 0.996 -> 0.945 us per sweep, same call).  What pointed here: the sweep's instruction mix replayed as a
// micro-benchmark issues at 3.26 cycles per wave-instruction and SIMD with its two v_mov_b32_dpp per row and at 2.27 with two
// ds_bpermute_b32 in their place (scripts/ubench/gen_block_bench.py, profiles/r03_block_replay.txt) -- in the kernel most of that
// difference does not show, and the column-layout kernel (8 shifts per thread and sweep) is SLOWER this way (EXPERIMENTS.md).
// `prev4` = 4 * ((lane - 1) & 63), held in a register by the caller; lane l + 1 is prev4 + 8 (the unit takes address bits 7:2).  Lane 0
// reads lane 63 and lane 63 lane 0 where DPP's bound_ctrl gave 0: both only ever meet a zero weight (sweep_tile_setup.inc: the right
// weight of a tile row's last pixel is 0, and lane 63 ends a tile row for every LX), and the values are finite.  The result arrives
// like an LDS read: the compiler waits on lgkmcnt before its first use.
__device__ __forceinline__ float lds_from_prev(int prev4, float v) { return __int_as_float(__builtin_amdgcn_ds_bpermute(prev4, __float_as_int(v))); }
__device__ __forceinline__ float lds_from_next(int prev4, float v) { return __int_as_float(__builtin_amdgcn_ds_bpermute(prev4 + 8, __float_as_int(v))); }

// The inter-workgroup hand-off's accesses (persist_sync.hpp).  Stores: write-through (sc1) 16-byte stores, no release fence needed -- the
// storing wave drains vmcnt itself.  Loads: 16-byte sc1 loads to registers (they bypass this CU's L1 and are served by L2 / memory): with
// EVERY load of handed-off bytes of this form, every store of them sc1 and drained, and the flag protocol of persist_sync.hpp, the consumer
// needs no agent-scope acquire (MI355X_MICROARCH.md, "Valid forms", table row 1).  Both take the address as a scalar base plus a 32-bit
// unsigned byte offset per lane (the instructions' `saddr` form): a kernel that exchanges the same rows many times keeps one offset per
// thread and forms no 64-bit address (sweep_blocked.hip).  Each statement opens with the wait states that a scalar base fresh from a
// v_readlane_b32 (an SGPR the compiler had spilled to a VGPR lane) needs before a VMEM instruction may read it -- 5; the compiler pads
// nothing inside a statement (persist_sync.hpp load_flag_at: the fault this comes from).  The halo statement's two scalar instructions
// in front of its first load count for two of them.
typedef float f4v_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_sc1_at(const float *base, uint32_t off, f4v_t v) {
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(off), "v"(v), "s"(base) : "memory");
}
// The halo loads of a thread's G rows from two planes, and the wait behind them, as ONE statement: row g is loaded (16 bytes from `bk`
// into a[g], 16 from `bm` into b[g], both at byte offset off[g]) in the lanes of mask[g]; the other lanes' registers, and rows whose
// mask is empty, keep their values.  a[] / b[] are read-write operands of the statement that also holds the s_waitcnt: whatever
// registers the compiler hands in are the ones that are loaded AND waited for, so no copy of a loaded register can come to lie between
// a load and the wait (two statements, loads and wait, leave the register allocator free to move a value in between -- it did, in the
// 168-register instantiations -- and such a copy reads stale bits).  tests/test_isa_hazards.py checks it on the disassembly all the same.
// EXEC is saved in front and put back behind, as in masked_fmac4 below; an SALU write of EXEC needs no wait state before a VMEM instruction.
#define RTDD_HALO_ROW(n) "s_and_b64 exec, %[sv], %[m" #n "]\n\tglobal_load_dwordx4 %[a" #n "], %[o" #n "], %[bk] sc1\n\tglobal_load_dwordx4 %[b" #n "], %[o" #n "], %[bm] sc1\n\t"
#define RTDD_HALO_OUT(n) [a##n] "+v"(a[n]), [b##n] "+v"(b[n])
#define RTDD_HALO_IN(n) [o##n] "v"(off[n]), [m##n] "s"(mask[n])
#define RTDD_HALO_ASM(rows, outs, ins) asm volatile("s_nop 2\n\ts_mov_b64 %[sv], exec\n\t" rows "s_mov_b64 exec, %[sv]\n\ts_waitcnt vmcnt(0)" : outs, [sv] "=&s"(sv) : ins, [bk] "s"(bk), [bm] "s"(bm) : "memory", "scc")
#define RTDD_C ,
template <int G>
__device__ __forceinline__ void load_halo_rows_sc1(f4v_t (&a)[G], f4v_t (&b)[G], const float *bk, const float *bm, const uint32_t (&off)[G], const unsigned long long (&mask)[G]) {
    unsigned long long sv;
    if constexpr (G == 1) RTDD_HALO_ASM(RTDD_HALO_ROW(0), RTDD_HALO_OUT(0), RTDD_HALO_IN(0));
    else if constexpr (G == 2) RTDD_HALO_ASM(RTDD_HALO_ROW(0) RTDD_HALO_ROW(1), RTDD_HALO_OUT(0) RTDD_C RTDD_HALO_OUT(1), RTDD_HALO_IN(0) RTDD_C RTDD_HALO_IN(1));
    else if constexpr (G == 3) RTDD_HALO_ASM(RTDD_HALO_ROW(0) RTDD_HALO_ROW(1) RTDD_HALO_ROW(2), RTDD_HALO_OUT(0) RTDD_C RTDD_HALO_OUT(1) RTDD_C RTDD_HALO_OUT(2),
                                             RTDD_HALO_IN(0) RTDD_C RTDD_HALO_IN(1) RTDD_C RTDD_HALO_IN(2));
    else if constexpr (G == 4) RTDD_HALO_ASM(RTDD_HALO_ROW(0) RTDD_HALO_ROW(1) RTDD_HALO_ROW(2) RTDD_HALO_ROW(3), RTDD_HALO_OUT(0) RTDD_C RTDD_HALO_OUT(1) RTDD_C RTDD_HALO_OUT(2) RTDD_C RTDD_HALO_OUT(3),
                                             RTDD_HALO_IN(0) RTDD_C RTDD_HALO_IN(1) RTDD_C RTDD_HALO_IN(2) RTDD_C RTDD_HALO_IN(3));
    else {
        static_assert(G == 6, "add a statement for this G");
        RTDD_HALO_ASM(RTDD_HALO_ROW(0) RTDD_HALO_ROW(1) RTDD_HALO_ROW(2) RTDD_HALO_ROW(3) RTDD_HALO_ROW(4) RTDD_HALO_ROW(5),
                      RTDD_HALO_OUT(0) RTDD_C RTDD_HALO_OUT(1) RTDD_C RTDD_HALO_OUT(2) RTDD_C RTDD_HALO_OUT(3) RTDD_C RTDD_HALO_OUT(4) RTDD_C RTDD_HALO_OUT(5),
                      RTDD_HALO_IN(0) RTDD_C RTDD_HALO_IN(1) RTDD_C RTDD_HALO_IN(2) RTDD_C RTDD_HALO_IN(3) RTDD_C RTDD_HALO_IN(4) RTDD_C RTDD_HALO_IN(5));
    }
}
#undef RTDD_C
#undef RTDD_HALO_ASM
#undef RTDD_HALO_IN
#undef RTDD_HALO_OUT
#undef RTDD_HALO_ROW

// Result stores: plain (non-temporal and write-through stores measured no faster: EXPERIMENTS.md).
__device__ __forceinline__ void store_result(float4 *p, float4 v) { *p = v; }

// ---- IEEE f32 division with a loop-invariant divisor ---------------------------------------------
// `sum / cnt` must be the correctly rounded quotient (the reference relies on nvcc's default
// -prec-div=true).  hipcc expands an IEEE divide into 11 VALU ops (v_div_scale x2, v_rcp, 5 fma,
// v_mul, v_div_fmas, v_div_fixup): measured 46 cycles per wave-instruction group, 60 % of a sweep.
// The divisor cnt is constant for a pixel, so its correctly rounded reciprocal y = RN(1/cnt) is
// computed once per launch (one full divide) and each sweep does Markstein's correction step
//      q0 = n*y;  r = fma(-d, q0, n);  q = fma(r, y, q0)
// which IS RN(n/d): verified EXHAUSTIVELY on gfx950 against hipcc's divide for all 2^23 divisor x 2^24
// numerator significands (scripts/ubench/div_exhaustive.hip, 1.4e14 pairs, 0 mismatches, 71 s; log in
// profiles/).  Powers of two scale every intermediate exactly, so that covers all operands for which no
// intermediate under/overflows: d normal (<= 4 here), n == 0 or |n| >= 2^-100 (then q0 is normal and the
// remainder, a multiple of 2^(e_n - 47), is exactly representable), n/d bounded (a weighted mean) and n finite: with n = +-inf, or a
// sum or n*y that overflows, fma(-d, inf, inf) is NaN where the IEEE quotient is +-inf, and the clamp behind it turns that NaN into 0
// and +inf into 255.
// Anything else leaves the 3-operation step under a wave-uniform branch.  Three guards send a wave there: a divisor below 2^-126 (tested
// per launch: the full divide), a numerator below 2^-100 (tested per group of rows, sweep_tile_sweeps.inc: div_tiny below, ten plain
// operations and no divide), and -- the upper end of the domain, the full divide again -- a solve
// whose INPUT holds a depth that is not finite or is 2^100 or more in magnitude: k_prepare reads every depth anyway and raises a
// launch-wide flag that every wave of the sweep kernels ORs into its choice (persist_sync.hpp kSyncWild, where it is also shown that
// an iterate that starts below that threshold never reaches an overflowing numerator).  Nothing per sweep.
__device__ __forceinline__ float div_tail(float n, float d, float y) {
    const float q0 = n * y;
    const float r = __builtin_fmaf(-d, q0, n);
    return __builtin_fmaf(r, y, q0);
}

// The quotient of a TINY numerator (|n| < 2^-100, denormals included; d normal and <= 4, y = RN(1/d)) without the 11-operation divide:
//      N  = n * 2^64                   exact, and inside div_tail's domain (2^-85 <= |N| < 2^-36, or 0)
//      qd = (N * y) * 2^-64            a first quotient ON THE QUOTIENT'S OWN GRID: the multiplication by 2^-64 rounds N * y to a
//                                      multiple of 2^-149 where the quotient is denormal and is exact where it is normal
//      R  = fma(-d, qd * 2^64, N)      the remainder of N against that grid point (qd * 2^64 is exact)
//      q  = fma(R, y * 2^-64, qd)      qd + R / d, rounded ONCE (y * 2^-64 is exact: y >= 1/4)
// This is div_tail's correction step carried out at the quotient's scale.  The form it replaces scaled back AFTER the correction and so
// rounded twice, to 24 bits and then to the 2^-149 grid: wrong wherever the 24-bit quotient sat on a midpoint of that grid, which it had
// to detect (a fifth of the denormal quotients) and hand to the IEEE divide.  Here the only rounding that sees the grid is the last one.
// Why R is exact: write g for the spacing of the quotient's grid at the scale of N (2^-85 where the quotient is denormal, its ulp
// otherwise) and Qd = qd * 2^64.  Qd is a multiple of g with at most 24 significant bits, d a multiple of ulp(d), N a multiple of
// 2^-85 and of its own ulp: so R = N - d * Qd is a multiple of ulp(d) * g, and as long as Qd is one of the two grid points next to N / d,
// |R| < |d| * g < 2^24 * ulp(d) * g -- it fits 24 bits and the fma returns it exactly (the usual exact-remainder argument, with g in the
// place of the quotient's ulp).  N * y is within 2^-23 of N / d relatively and the rounding to the grid adds half a step, so Qd IS such
// a neighbour except possibly in the top binade of the denormal range with a divisor significand close to 2, where the bound on
// |Qd - N / d| is 1.25 g rather than g; R may then need a 25th bit and is rounded by 2^-25 of itself, far below what moves the result
// across a midpoint -- that corner is covered by the exhaustive run, not by this argument.  Why the last fma rounds once, to the right
// grid: qd is on the grid, |R * y * 2^-64| is about a step or less, the exact sum qd + R / d is n / d up to y's relative error 2^-24 applied
// to the CORRECTION only (2^-24 of a step), and the fma rounds that sum directly to f32 -- which, for a denormal result, IS the 2^-149 grid.
// The scale is per lane: 2^64 where the numerator is tiny and 1 elsewhere (n * 2^64 could overflow there), so that a lane that is not
// tiny gets div_tail(n, d, y) again, operation for operation -- the valid quotient it already had.  The caller needs no select, keeps no
// earlier quotient alive across the branch and has no second branch behind it.  Ten VALU operations, none of them quarter rate.
// The multiplications by 2^+-64 need f32 denormals honoured, as the whole solve does.  Checked against hipcc's divide on gfx950 for all
// 2^23 divisor significands and every underflow depth of the quotient: scripts/ubench/div_tiny_exhaustive.hip, log in profiles/;
// restated in C in tests/test_div_tiny_once_cpu.py (tests/test_div_tiny_cpu.py keeps the two-rounding form and its suspects on record).
__device__ __forceinline__ float div_tiny(float n, float d, float y) {
    const bool tiny = __builtin_fabsf(n) < 0x1p-100f;            // (a zero numerator: +0 either way)
    const float up = tiny ? 0x1p64f : 1.0f, down = tiny ? 0x1p-64f : 1.0f;
    const float N = n * up;
    const float qd = (N * y) * down;
    const float R = __builtin_fmaf(-d, qd * up, N);
    return __builtin_fmaf(R, y * down, qd);
}

// div_tiny with the scale a CONSTANT, 2^64 in every lane: the quotient of ANY numerator with |n| < 2^64 (zero and the denormals included;
// d normal, y = RN(1/d), the quotient a bounded mean as above), rounded once.  No test in front of it, no fast attempt, no select:
//   * |n| < 2^-100: operation for operation what div_tiny does in a tiny lane, proven there;
//   * an ordinary numerator: n * 2^64 is exact (this is where |n| < 2^64 is needed: it must not overflow), N * y rounds to 24 bits and its
//     multiplication by 2^-64 is exact wherever the quotient is normal, so qd IS div_tail's q0, R is 2^64 times div_tail's remainder --
//     exact, the same argument -- and the last fma rounds qd + R * y / 2^64 = q0 + r * y once: Markstein's step itself;
//   * in between (a quotient in or next to the denormals from a numerator of 2^-100 or more) it is div_tiny's argument again: the first
//     quotient lies on the quotient's own grid, the remainder against it is exact, the last fma is the only rounding that sees the grid.
// Seven full-rate operations, the constants literals of the multiplications.  Who may use it: the persistent sweep's waves in scaled mode
// (sweep_blocked.hip), in a solve whose input holds no depth of 2^32 or more (persist_sync.hpp kSyncLarge, where the bound on the numerator
// is derived).  Restated in C and checked against the IEEE divide in tests/test_div_scaled_cpu.py, on gfx950 by
// scripts/ubench/div_scaled_exhaustive.hip.
__device__ __forceinline__ float div_scaled(float n, float d, float y) {
    const float N = n * 0x1p64f;
    const float qd = (N * y) * 0x1p-64f;
    const float R = __builtin_fmaf(-d, qd * 0x1p64f, N);
    return __builtin_fmaf(R, y * 0x1p-64f, qd);
}

// div_scaled in FOUR operations, with the two per-pixel constants stored in scaled form: D = d * 2^64 in place of the divisor and
// ys = y * 2^-64 in place of its reciprocal.  It replaces div_scaled in the tile that enters scaled mode at the start (sweep_blocked.hip
// kFromStart, sweep_tile_sweeps.inc MODE == 2); the tiles that enter on demand keep div_scaled, above, which is also the form this one is
// derived from and checked against (tests/test_div_scaled_cpu.py).
//      N  = n * 2^64               exact for |n| < 2^64
//      qd = N * ys                 = RN(n * y): ONE rounding, to 24 bits where the quotient is normal and to the 2^-149 grid where it is not
//      R  = fma(-D, qd, N)         = 2^64 * (n - d * qd)
//      q  = fma(R, ys, qd)         = RN(qd + (n - d * qd) * y): the only rounding that sees the result's grid
// Domain: |n| < 2^64 (persist_sync.hpp kSyncLarge), d normal and <= 4, y = RN(1/d), the quotient a bounded mean.  Then both conversions
// are exact and stay normal: D <= 2^66, and 2^-66 <= ys <= 2^62 because 1/4 <= y <= 2^126.  They are made once, behind the tile setup, where the
// wave enters scaled mode (sweep_blocked.hip); a wave of the IEEE variant (a denormal divisor) never converts.
// Against div_scaled, operation by operation: N is the same number.  -D * qd is, exactly, -d * (qd * 2^64) -- div_scaled's product, whose
// factor qd * 2^64 is exact -- so R is the same fma of the same three real numbers GIVEN THE SAME qd; likewise the last fma (ys is
// div_scaled's y * 2^-64, exact).  The one difference is qd: div_scaled rounds N * y to 24 bits and then, multiplying by 2^-64, to the
// quotient's grid (twice where the quotient is denormal); here N * ys is the real number n * y rounded to that grid once.
//   * the quotient normal (every ordinary numerator, |n| >= 2^-100 included): the grid IS 24 bits, both forms give qd = RN(n * y) = div_tail's
//     q0, R = 2^64 * div_tail's r, exact by the usual argument, and the last fma is Markstein's: the same bits as div_tail and div_scaled;
//   * the quotient denormal or next to it: div_tiny's argument needs of qd only that it lies ON the quotient's grid and is one of the two
//     grid points next to N / d, so that R = N - d * Qd (Qd = qd * 2^64, a multiple of the step g with at most 24 bits) is a multiple of
//     ulp(d) * g below 2^24 * ulp(d) * g and the fma returns it exactly.  Here n * y is off n / d by y's rounding alone, 2^-24 of a
//     quotient of fewer than 2^23 steps: under half a step; the single rounding to the grid adds at most half a step.  So |Qd - N / d| < g
//     for EVERY denormal quotient -- the double rounding's extra half ulp, which left div_tiny's argument the top denormal binade as a
//     corner for the exhaustive run, is gone.  The two forms can differ only in WHICH neighbour they start from; the last fma adds the
//     exact remainder over d to either and rounds the same real number, n / d up to 2^-24 of a step, once.
// A zero numerator of either sign gives +0, as div_tail does.  Four full-rate operations, the 2^64 a literal of the first multiplication
// (scripts/isa_count.py finds the scaled sweep pair by it); no register more than div_tail's three operands.  Restated in C and checked
// against the IEEE divide, div_scaled and div_tail in tests/test_div_scaled4_cpu.py; on gfx950 by scripts/ubench/div_scaled4_exhaustive.hip.
// The numerator's chain WITHOUT its leading `0 +` (sweep_tile_sweeps.inc wsum, this tile's scaled pair only).  Every other sweep starts a
// pixel's sum as 0 + p, p the left term (weight times value, a rounded product or the first fma's), and adds the other three terms; here
// the chain starts at p itself -- an addition less per row with contraction, per pixel without.  Why no quotient changes:
//   * 0 + p differs from p only for p = -0, where it is +0;
//   * a -0 in the place of a +0 addend changes a later partial sum only while every product added so far is an exact zero (a nonzero
//     product, however it rounds, gives the same sum with either zero), and then only that sum's sign: (-0) + (-0) = -0 where
//     (+0) + (-0) = +0, as an addition or inside an fma;
//   * so the chain's result differs at most by being -0 in place of +0;
//   * and div_scaled4 gives +0 for both: N = -+0, qd = -+0 (ys > 0), R = fma(-D, qd, N) = (+-0) + (-+0) = +0 in round-to-nearest,
//     q = fma(+0, ys, -+0) = +0 + -+0 = +0.
// The IEEE variant (-0 / d = -0 there) and the fast variant keep the addition.  Restated from the sources and compared bit for bit, both contraction forms, in tests/test_div_scaled4_signed_zero_cpu.py.
__device__ __forceinline__ float div_scaled4(float n, float D, float ys) {
    const float N = n * 0x1p64f;
    const float qd = N * ys;
    const float R = __builtin_fmaf(-D, qd, N);
    return __builtin_fmaf(R, ys, qd);
}

// fma(a, b, c) as ONE three-address v_fma_f32, all operands in VGPRs.  For an fma whose addend stays live behind it (the update's
// fma(gamma, r - x, x): x is read again by the next sweep) the compiler picks between that and a copy of the addend plus the two-address
// v_fmac_f32; in one of the six rows of the from-start tile's scaled pair -- the row whose sweep straddles the loop's back edge -- it took the
// copy, one v_mov_b32 per pixel.  The same operation on the same operands, rounded once.
__device__ __forceinline__ float fma_vvv(float a, float b, float c) {
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// RN(1/d) for a normal d with a normal reciprocal: v_rcp_f32 (1 ulp) + one Newton step.  Equal to the IEEE quotient 1.0f/d for
// EVERY such f32 (all 4 227 858 434 of them checked on the GPU, scripts/ubench/rcp_exhaustive.hip, profiles/r01_rcp_exhaustive.log):
// 3 VALU ops instead of the 11 of the full divide, in the per-launch setup of every pixel.
__device__ __forceinline__ float rcp_rn(float d) {
    const float y0 = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, y0, 1.0f), y0, y0);
}

// ---- the last operation of a pixel's update under an EXEC mask ----------------------------------------------------------------
// x_{k+1} = fma(omega, t, x_{k-1}) overwrites x_{k-1}'s register -- for FREE pixels only; a Dirichlet pixel keeps its value, and its
// register holds that value in both iterates (k_prepare stores it in both planes, sweep_tile_setup.inc enforces it on the tile).  So
// the select of `(dirichlet ? x : v)` -- a v_cndmask_b32 with an SGPR-pair mask, half rate on gfx950 (4.4 cycles per wave-instruction
// against 3.1 for v_fmac_f32 with three VGPRs and 4.3 for any fma with an SGPR operand: scripts/ubench/excp_probe.hip,
// profiles/r05_excp_probe.txt) -- becomes the EXEC mask of the fma itself: s_mov_b64 exec (scalar unit) + v_fmac_f32 (full rate), omega
// in a VGPR.  ONE asm statement per row so that the compiler can schedule nothing between the EXEC writes.  Round 6: the
// statement no longer ASSUMES that EXEC is all ones on entry (true today: every thread of the whole-wave workgroup runs the sweeps and
// all control flow around them is wave-uniform -- but a compiler that sank the statement into a divergent region would have had its
// inactive lanes switched on by the old closing `s_mov_b64 exec, -1`): the first mask is applied by s_and_saveexec_b64, which also SAVES
// the entry EXEC; the other masks are `entry & mask`; the last instruction puts the entry EXEC back.  Same five scalar instructions per
// row as before, one SGPR pair more for the duration of the statement.  An SALU write of EXEC needs no wait state in front of a
// (non-DPP) VALU instruction on gfx9.
__device__ __forceinline__ void masked_fmac4(float &o0, float &o1, float &o2, float &o3, float w, float t0, float t1, float t2, float t3,
                                             unsigned long long m0, unsigned long long m1, unsigned long long m2, unsigned long long m3) {
    unsigned long long entry;                // EXEC as it was on entry: saved by the instruction that applies the first mask, put back by the last
    asm("s_and_saveexec_b64 %[e], %[m0]\n\tv_fmac_f32_e32 %[o0], %[w], %[t0]\n\t"
        "s_and_b64 exec, %[e], %[m1]\n\tv_fmac_f32_e32 %[o1], %[w], %[t1]\n\t"
        "s_and_b64 exec, %[e], %[m2]\n\tv_fmac_f32_e32 %[o2], %[w], %[t2]\n\t"
        "s_and_b64 exec, %[e], %[m3]\n\tv_fmac_f32_e32 %[o3], %[w], %[t3]\n\t"
        "s_mov_b64 exec, %[e]"
        : [o0] "+v"(o0), [o1] "+v"(o1), [o2] "+v"(o2), [o3] "+v"(o3), [e] "=&s"(entry)
        : [w] "v"(w), [t0] "v"(t0), [t1] "v"(t1), [t2] "v"(t2), [t3] "v"(t3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3)
        : "scc");
}
// the same for the un-contracted update, (omega * t) + x_{k-1}: the product is formed outside, the addition is masked
__device__ __forceinline__ void masked_add4(float &o0, float &o1, float &o2, float &o3, float p0, float p1, float p2, float p3,
                                            unsigned long long m0, unsigned long long m1, unsigned long long m2, unsigned long long m3) {
    unsigned long long entry;
    asm("s_and_saveexec_b64 %[e], %[m0]\n\tv_add_f32_e32 %[o0], %[p0], %[o0]\n\t"
        "s_and_b64 exec, %[e], %[m1]\n\tv_add_f32_e32 %[o1], %[p1], %[o1]\n\t"
        "s_and_b64 exec, %[e], %[m2]\n\tv_add_f32_e32 %[o2], %[p2], %[o2]\n\t"
        "s_and_b64 exec, %[e], %[m3]\n\tv_add_f32_e32 %[o3], %[p3], %[o3]\n\t"
        "s_mov_b64 exec, %[e]"
        : [o0] "+v"(o0), [o1] "+v"(o1), [o2] "+v"(o2), [o3] "+v"(o3), [e] "=&s"(entry)
        : [p0] "v"(p0), [p1] "v"(p1), [p2] "v"(p2), [p3] "v"(p3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3)
        : "scc");
}

}  // namespace rtdd
