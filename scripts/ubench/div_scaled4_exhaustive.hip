// Exhaustive check (gfx950) of div_scaled4 (csrc/sweep_common.hpp), the four-operation divide of a persistent wave in scaled mode, which
// holds its per-pixel constants as D = d * 2^64 and ys = y * 2^-64: for EVERY numerator with |n| < 2^64, tiny or not,
//     N = n * 2^64;  qd = N * ys;  R = fma(-D, qd, N);  q = fma(R, ys, qd)        with  y = RN(1/d)  (IEEE 1.0f/d)
// is bit-identical to the IEEE-754 correctly rounded n/d (hipcc's `/` with -fhip-fp32-correctly-rounded-divide-sqrt): 0 mismatches is
// the requirement.  For the record it also counts the pairs that differ from div_scaled, the seven-operation form it replaces (none),
// and, among the pairs whose numerator is 2^-100 or more and whose quotient is normal -- the 3-operation divide's domain -- those that
// differ from div_tail (none: there the step is Markstein's own).
// Coverage as div_scaled_exhaustive.hip.  Divisors: all 2^23 significands, in both binades [1,2) and [2,4), plus 4.0 itself with the first
// significand.  Numerators, per divisor, in EVERY binade from 2^-149 up to 2^63 -- the 23 denormal ones, split by their leading bit, and the
// 190 normal ones --: 2^11 few-bit significands (the top 11 bits, the rest zero) and 2^11 seeded full-width ones; signs alternate.
// 8.7e5 numerators per divisor of either binade, 1.46e13 pairs.
// build: hipcc --offload-arch=gfx950 -O3 -fhip-fp32-correctly-rounded-divide-sqrt -o div_scaled4_exhaustive div_scaled4_exhaustive.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
__device__ __forceinline__ float div_tail(float n, float d, float y) {
    const float q0 = n * y;
    const float r = __builtin_fmaf(-d, q0, n);
    return __builtin_fmaf(r, y, q0);
}
__device__ __forceinline__ float div_scaled(float n, float d, float y) {
    const float N = n * 0x1p64f;
    const float qd = (N * y) * 0x1p-64f;
    const float R = __builtin_fmaf(-d, qd * 0x1p64f, N);
    return __builtin_fmaf(R, y * 0x1p-64f, qd);
}
__device__ __forceinline__ float div_scaled4(float n, float D, float ys) {
    const float N = n * 0x1p64f;
    const float qd = N * ys;
    const float R = __builtin_fmaf(-D, qd, N);
    return __builtin_fmaf(R, ys, qd);
}
struct Counts { unsigned long long pairs, bad, denormal_q, tiny_n, ordinary, tail_differs, scaled_differs; };
__device__ void one(uint32_t nbits, float d, float y, float D, float ys, Counts &c, unsigned *example) {
    const float n = __uint_as_float(nbits);
    if ((nbits << 1) == 0) return;
    const float want = n / d;
    const float got = div_scaled4(n, D, ys);
    c.pairs++;
    if (__builtin_fabsf(want) < 0x1p-126f) c.denormal_q++;
    if (__builtin_fabsf(n) < 0x1p-100f) c.tiny_n++;
    else if (__builtin_fabsf(want) >= 0x1p-126f) { c.ordinary++; c.tail_differs += __float_as_uint(got) != __float_as_uint(div_tail(n, d, y)); }
    c.scaled_differs += __float_as_uint(got) != __float_as_uint(div_scaled(n, d, y));
    if (__float_as_uint(got) != __float_as_uint(want)) {
        c.bad++;
        if (atomicAdd(&example[0], 1u) == 0) { example[1] = nbits; example[2] = __float_as_uint(d); example[3] = __float_as_uint(got); }
    }
}
__global__ void k(unsigned d_begin, unsigned d_count, unsigned long long *counters, unsigned *example) {
    const unsigned di = d_begin + blockIdx.x;
    if (blockIdx.x >= d_count) return;
    Counts c = {};
    unsigned rng = di * 2654435761u + threadIdx.x * 40503u + 1u;
    const int nd = di == 0 ? 3 : 2;                                        // significand 0: 1.0, 2.0 and 4.0
    for (int b = 0; b < nd; b++) {
        const float d = __uint_as_float(((127u + b) << 23) | di);
        const float y = 1.0f / d;
        const float D = d * 0x1p64f, ys = y * 0x1p-64f;                    // the conversion a wave makes where it enters the mode
        for (unsigned j = threadIdx.x; j < (1u << 12); j += blockDim.x) {
            uint32_t sig;
            if (j < (1u << 11)) sig = j << 12;                             // few-bit
            else { rng = rng * 1664525u + 1013904223u; sig = (rng >> 9) & 0x7FFFFFu; }
            const uint32_t sign = (j & 1u) << 31;
            for (uint32_t e = 1; e <= 190; e++) one(sign | (e << 23) | sig, d, y, D, ys, c, example);        // 2^-126 .. 2^63
            for (int lead = 0; lead < 23; lead++) one(sign | (((1u << 23) | sig) >> (23 - lead)), d, y, D, ys, c, example);      // denormals with leading bit `lead`
        }
    }
    atomicAdd(&counters[0], c.pairs);
    if (c.bad) atomicAdd(&counters[1], c.bad);
    if (c.denormal_q) atomicAdd(&counters[2], c.denormal_q);
    if (c.tiny_n) atomicAdd(&counters[3], c.tiny_n);
    if (c.ordinary) atomicAdd(&counters[4], c.ordinary);
    if (c.tail_differs) atomicAdd(&counters[5], c.tail_differs);
    if (c.scaled_differs) atomicAdd(&counters[6], c.scaled_differs);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
int main(int argc, char **argv) {
    const unsigned total = argc > 1 ? (unsigned)atol(argv[1]) : (1u << 23);     // number of divisor significands to cover
    unsigned long long *counters; unsigned *ex;
    CK(hipMalloc(&counters, 64)); CK(hipMalloc(&ex, 16)); CK(hipMemset(counters, 0, 64)); CK(hipMemset(ex, 0, 16));
    const unsigned chunk = 1u << 16;
    for (unsigned b = 0; b < total; b += chunk) {
        const unsigned cnt = total - b < chunk ? total - b : chunk;
        // stride the chunks over the whole significand range when only a subset is requested
        const unsigned begin = total == (1u << 23) ? b : (unsigned)(((unsigned long long)b << 23) / total);
        k<<<cnt, 256>>>(begin, cnt, counters, ex);
        CK(hipDeviceSynchronize());
        if ((b / chunk) % 8 == 0) { printf("progress %u / %u divisors\n", b + cnt, total); fflush(stdout); }
    }
    unsigned long long h[8]; unsigned hex[4];
    CK(hipMemcpy(h, counters, 64, hipMemcpyDeviceToHost)); CK(hipMemcpy(hex, ex, 16, hipMemcpyDeviceToHost));
    printf("divisor significands %u x 2 binades, numerators in the 213 binades 2^-149 .. 2^63, pairs %llu (tiny numerators %llu, denormal quotients %llu): mismatches = %llu; "
           "different from div_scaled = %llu; pairs in the 3-operation divide's domain %llu, of them different from div_tail = %llu\n", total, h[0], h[3], h[2], h[1], h[6], h[4], h[5]);
    if (h[1]) printf("first mismatch: n = 0x%08x d = 0x%08x got 0x%08x\n", hex[1], hex[2], hex[3]);
    return h[1] || h[5] || h[6] ? 1 : 0;
}
