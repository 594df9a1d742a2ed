// Exhaustive check (gfx950) of div_tiny (csrc/sweep_common.hpp), the one-rounding form: for a numerator 0 < |n| < 2^-100,
//     N = n * 2^64;  qd = (N * y) * 2^-64;  R = fma(-d, qd * 2^64, N);  q = fma(R, y * 2^-64, qd)        with  y = RN(1/d)  (IEEE 1.0f/d)
// is bit-identical to the IEEE-754 correctly rounded n/d (hipcc's `/` with -fhip-fp32-correctly-rounded-divide-sqrt) in EVERY lane: 0
// mismatches is the requirement, full stop.  For the record it also counts the pairs that the two-rounding form before it
// (Q = div_tail(N, d, y); q = Q * 2^-64) called suspect (Q on a midpoint of the 2^-149 grid) and those of them that form got wrong.
// It also shows that the multiplications by 2^+-64 honour f32 denormals in the mode the kernels are compiled for.
// Divisors: all 2^23 significands, in both binades [1,2) and [2,4) (a denormal quotient does not scale with the divisor's binade: the
// numerator cannot follow below 2^-149), plus 4.0 itself with the first significand.  Numerators, per divisor, in EVERY binade below
// 2^-100 -- the 26 normal ones and the denormals, which are split by their leading bit into 23 more -- 2^13 few-bit significands (the
// top 13 bits, the rest zero), 2^13 seeded full-width ones and, among the denormals, every one below 2^12; signs alternate.  The
// quotient's underflow depth runs from 0 (normal) to 25 binades (n = 2^-149, d > 2: rounds to zero).  8.1e5 numerators per divisor
// and binade, 1.35e13 pairs.  Divisors below 1 scale every intermediate exactly (the numerator follows upwards).
// build: hipcc --offload-arch=gfx950 -O3 -fhip-fp32-correctly-rounded-divide-sqrt -o div_tiny_exhaustive div_tiny_exhaustive.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
__device__ __forceinline__ float div_tail(float n, float d, float y) {
    const float q0 = n * y;
    const float r = __builtin_fmaf(-d, q0, n);
    return __builtin_fmaf(r, y, q0);
}
__device__ __forceinline__ float div_tiny(float n, float d, float y) {
    const bool tiny = __builtin_fabsf(n) < 0x1p-100f;
    const float up = tiny ? 0x1p64f : 1.0f, down = tiny ? 0x1p-64f : 1.0f;
    const float N = n * up;
    const float qd = (N * y) * down;
    const float R = __builtin_fmaf(-d, qd * up, N);
    return __builtin_fmaf(R, y * down, qd);
}
// the two-rounding form, for the census of what it could not do
__device__ __forceinline__ float div_tiny_twice(float n, float d, float y, bool &suspect) {
    const float N = n * 0x1p64f;
    const float Q = div_tail(N, d, y);
    const float q = Q * 0x1p-64f;
    suspect = __builtin_fabsf(__builtin_fmaf(q, -0x1p64f, Q)) == 0x1p-86f;
    return q;
}
struct Counts { unsigned long long pairs, bad, suspects, suspects_differ, denormal_q, tie_bad, deepest; };
__device__ void one(uint32_t nbits, float d, float y, Counts &c, unsigned *example) {
    const float n = __uint_as_float(nbits);
    if ((nbits << 1) == 0 || (nbits << 1) >= (27u << 24)) return;         // 0 < |n| < 2^-100
    const float want = n / d;
    bool s;
    const float got = div_tiny(n, d, y);
    const float old = div_tiny_twice(n, d, y, s);
    c.pairs++;
    if (__builtin_fabsf(want) < 0x1p-126f) c.denormal_q++;
    if (want == 0.0f) c.deepest++;
    const bool differ = __float_as_uint(got) != __float_as_uint(want);
    if (s) { c.suspects++; c.suspects_differ += __float_as_uint(old) != __float_as_uint(want); c.tie_bad += differ; }
    if (differ) {
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
        for (unsigned j = threadIdx.x; j < (1u << 14); j += blockDim.x) {
            uint32_t sig;
            if (j < (1u << 13)) sig = j << 10;                             // few-bit
            else { rng = rng * 1664525u + 1013904223u; sig = (rng >> 9) & 0x7FFFFFu; }
            const uint32_t sign = (j & 1u) << 31;
            for (uint32_t e = 1; e <= 26; e++) one(sign | (e << 23) | sig, d, y, c, example);         // the normal binades below 2^-100
            for (int lead = 0; lead < 23; lead++) one(sign | (((1u << 23) | sig) >> (23 - lead)), d, y, c, example);      // denormals with leading bit `lead`
            if (j < (1u << 12)) one(sign | j, d, y, c, example);           // the deepest denormals, every one
        }
    }
    atomicAdd(&counters[0], c.pairs);
    if (c.bad) atomicAdd(&counters[1], c.bad);
    if (c.suspects) atomicAdd(&counters[2], c.suspects);
    if (c.suspects_differ) atomicAdd(&counters[3], c.suspects_differ);
    if (c.denormal_q) atomicAdd(&counters[4], c.denormal_q);
    if (c.tie_bad) atomicAdd(&counters[5], c.tie_bad);
    if (c.deepest) atomicAdd(&counters[6], c.deepest);
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
    printf("divisor significands %u x 2 binades, pairs %llu (denormal quotients %llu, quotients that round to zero %llu): mismatches = %llu; "
           "for the record, the two-rounding form's suspects = %llu (%.3f %% of the pairs, %.1f %% of the denormal quotients), of them wrong in that form = %llu, wrong in this one = %llu\n",
           total, h[0], h[4], h[6], h[1], h[2], 100.0 * h[2] / (h[0] ? h[0] : 1), 100.0 * h[2] / (h[4] ? h[4] : 1), h[3], h[5]);
    if (h[1]) printf("first mismatch: n = 0x%08x d = 0x%08x got 0x%08x\n", hex[1], hex[2], hex[3]);
    return h[1] || h[5] ? 1 : 0;
}
