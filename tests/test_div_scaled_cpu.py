"""div_scaled (csrc/sweep_common.hpp), the divide of a persistent wave in scaled mode, compared with the host's IEEE divide.

    N = n * 2^64;  qd = (N * y) * 2^-64;  R = fma(-d, qd * 2^64, N);  q = fma(R, y * 2^-64, qd)            y = RN(1/d), d normal

It is div_tiny (tests/test_div_tiny_once_cpu.py) with the scale a constant, used for EVERY numerator of the wave: tiny ones, for which it
is what div_tiny does, and ordinary ones, for which the scaling is exact and the step is the 3-operation divide's own.  Its domain is
|n| < 2^64 (n * 2^64 must not overflow) with a bounded quotient (a weighted mean: persist_sync.hpp kSyncLarge).

The function is not restated here: its text is cut out of sweep_common.hpp and compiled as C (the builtins it uses are the host
compiler's too), without contraction.  Required: 0 differences from `/`, over

  * every divisor significand, all 2^23 in [1, 2) and all 2^23 in [2, 4), each with 8 numerators drawn (seeded) from the 213 binades from
    2^-149 (the 23 denormal ones included) up to 2^63, the binades taken in turn so that each gets the same share, both signs;
  * a zero numerator of either sign with every one of those divisors: the quotient is +0, which is what div_tail answers too (IEEE
    gives -0 / d = -0; the clamp to [0, 255] behind the divide makes nothing of the difference);
  * divisors near 2^-126 (the smallest normal ones: 2^16 significands from 2^-126 up, and the top of that binade) with numerators from
    2^-149 up to 2^34 times the divisor -- in a solve a numerator is at most the divisor times the largest iterate;
  * divisors near 2^2 (4 is the largest a solve can hold: four weights of 1): the 2^12 floats on either side of 4, every binade again.

Where the numerator is 2^-100 or more and the quotient is normal the result must also be div_tail's, bit for bit.  A few seconds."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPP = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc", "sweep_common.hpp")

MAIN = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define __device__
#define __forceinline__ static inline
%s
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float fl(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
#define BINADES 213                            /* exponent fields 0 (denormals: 23 binades, 2^-149 .. 2^-127) and 1 .. 190 (2^-126 .. 2^63) */
static unsigned long long total, bad, denormal_q, tiny_n, ordinary, tail_differs, zero_bad, first_n, first_d, per_binade[BINADES];
static float numerator(int binade) {           /* a seeded numerator of that binade, either sign */
    uint32_t nb;
    if (binade < 23) { nb = 1u << binade; nb |= rnd() & (nb - 1u); }             /* denormal: leading bit at `binade` */
    else nb = ((uint32_t)(binade - 22) << 23) | (rnd() & 0x007FFFFFu);
    if (rnd() & 1) nb |= 0x80000000u;
    return fl(nb);
}
static void one(float n, float d, int binade) {
    volatile float vn = n, vd = d;
    float want = vn / vd, y = 1.0f / vd;
    float got = div_scaled(n, d, y);
    total++;
    if (binade >= 0) per_binade[binade]++;
    if (fabsf(want) < 0x1p-126f && want != 0.0f) denormal_q++;
    if (fabsf(n) < 0x1p-100f) tiny_n++;
    else if (fabsf(want) >= 0x1p-126f) { ordinary++; tail_differs += bits(got) != bits(div_tail(n, d, y)); }
    if (bits(got) != bits(want)) { if (!bad) { first_n = bits(n); first_d = bits(d); } bad++; }
}
int main(void) {
    int turn = 0;
    /* every significand of [1, 2) and [2, 4) */
    for (uint32_t db = 0x3F800000u; db < 0x40800000u; db++) {
        float d = fl(db);
        for (int k = 0; k < 8; k++) { one(numerator(turn), d, turn); turn = (turn + 1) %% BINADES; }
        volatile float vd = d;
        float y = 1.0f / vd;
        /* (+0 for a zero of either sign, as div_tail gives it: the clamp behind the divide does not tell the two zeros apart) */
        zero_bad += bits(div_scaled(0.0f, d, y)) != 0u || bits(div_scaled(-0.0f, d, y)) != bits(div_tail(-0.0f, d, y)) || bits(div_tail(-0.0f, d, y)) != 0u;
    }
    /* near 2^-126: numerators up to 2^34 times the divisor (exponent field 1 + 34 -> binades 0 .. 57) */
    for (uint32_t i = 0; i < (1u << 16); i++) {
        const float ds[3] = {fl(0x00800000u + i), fl(0x00FFFFFFu - i), fl(0x00800000u + (rnd() & 0x007FFFFFu))};
        for (int j = 0; j < 3; j++)
            for (int b = 0; b < 58; b += 1 + (int)(rnd() %% 3)) one(numerator(b), ds[j], -1);
    }
    /* near 2^2 */
    for (uint32_t i = 0; i < (1u << 12); i++) {
        const float ds[2] = {fl(0x40800000u + i), fl(0x40800000u - 1u - i)};
        for (int j = 0; j < 2; j++)
            for (int b = 0; b < BINADES; b++) one(numerator(b), ds[j], -1);
    }
    unsigned long long least = ~0ull;
    for (int b = 0; b < BINADES; b++) if (per_binade[b] < least) least = per_binade[b];
    printf("%%llu %%llu %%llu %%llu %%llu %%llu %%llu %%llu %%08llx %%08llx\n", total, bad, denormal_q, tiny_n, ordinary, tail_differs, zero_bad, least, first_n, first_d);
    return 0;
}
"""


def _device_function(name):
    """The text of a `__device__ __forceinline__ float name(...) { ... }` of sweep_common.hpp, as it stands."""
    text = open(HPP).read()
    m = re.search(r"^__device__ __forceinline__ float " + name + r"\(.*?^}\n", text, re.S | re.M)
    assert m, name
    return m.group(0)


def test_div_scaled_is_the_ieee_quotient(tmp_path):
    src = tmp_path / "div_scaled.c"
    exe = tmp_path / "div_scaled"
    src.write_text(MAIN % (_device_function("div_tail") + _device_function("div_scaled")))
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)], text=True).split()
    total, bad, denormal_q, tiny_n, ordinary, tail_differs, zero_bad, least = (int(v) for v in out[:8])
    print(f"pairs {total} (at least {least} in each of the 213 binades 2^-149 .. 2^63), differences {bad} (first n = 0x{out[8]}, d = 0x{out[9]}); "
          f"denormal quotients {denormal_q}, tiny numerators {tiny_n}; ordinary pairs {ordinary}, of them different from div_tail {tail_differs}; "
          f"zero numerators wrong {zero_bad}")
    assert total > 130_000_000 and least >= 600_000 and denormal_q > 5_000_000 and tiny_n > 20_000_000
    assert ordinary > 80_000_000 and tail_differs == 0           # an ordinary numerator: the 3-operation divide's own result
    assert zero_bad == 0
    assert bad == 0
