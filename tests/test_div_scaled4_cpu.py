"""div_scaled4 (csrc/sweep_common.hpp), the four-operation divide of a persistent wave in scaled mode, compared with the host's IEEE divide.

    N = n * 2^64;  qd = N * ys;  R = fma(-D, qd, N);  q = fma(R, ys, qd)            D = d * 2^64, ys = RN(1/d) * 2^-64, d normal and <= 4

It is div_scaled (tests/test_div_scaled_cpu.py) with the per-pixel constants stored in scaled form, which saves the three multiplications
that moved between the scales and rounds the first quotient once instead of twice.  Its domain is div_scaled's: |n| < 2^64 with a bounded
quotient (a weighted mean: persist_sync.hpp kSyncLarge).

The function is not restated here: its text is cut out of sweep_common.hpp and compiled as C (the builtins it uses are the host
compiler's too), without contraction, next to div_scaled's and div_tail's.  The conversion of the constants is made the way the kernel
makes it, by two multiplications.  Required: 0 differences from `/`, over

  * every divisor significand, all 2^23 in [1, 2) and all 2^23 in [2, 4), each with 6 numerators drawn (seeded) from the 213 binades from
    2^-149 (the 23 denormal ones included) up to 2^63, the binades taken in turn so that each gets the same share, both signs;
  * a zero numerator of either sign with every one of those divisors: the quotient is +0, which is what div_tail answers too (IEEE
    gives -0 / d = -0; the clamp to [0, 255] behind the divide makes nothing of the difference);
  * divisors ACROSS [2^-126, 4): every one of the 128 binades in turn, seeded significands, with numerators from 2^-149 up to 2^34 times
    the divisor -- in a solve a numerator is at most the divisor times the largest iterate, and the quotient must stay finite;
  * divisors near 2^-126 (the smallest normal ones: 2^16 significands from 2^-126 up, and the top of that binade), numerators as above;
  * divisors near 2 and near 2^2 (4 is the largest a solve can hold: four weights of 1): the 2^12 floats on either side of each, every
    binade of the numerator again.

On every pair the result must also be div_scaled's, and where the numerator is 2^-100 or more and the quotient is normal div_tail's, bit for
bit.  A few seconds."""
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
static unsigned long long total, bad, denormal_q, tiny_n, ordinary, tail_differs, scaled_differs, zero_bad, small_d, first_n, first_d, per_binade[BINADES];
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
    volatile float D = d * 0x1p64f, ys = y * 0x1p-64f;         /* the conversion, as the kernel makes it */
    float got = div_scaled4(n, D, ys);
    total++;
    if (binade >= 0) per_binade[binade]++;
    if (fabsf(want) < 0x1p-126f && want != 0.0f) denormal_q++;
    if (fabsf(n) < 0x1p-100f) tiny_n++;
    else if (fabsf(want) >= 0x1p-126f) { ordinary++; tail_differs += bits(got) != bits(div_tail(n, d, y)); }
    scaled_differs += bits(got) != bits(div_scaled(n, d, y));
    if (bits(got) != bits(want)) { if (!bad) { first_n = bits(n); first_d = bits(d); } bad++; }
}
int main(void) {
    int turn = 0;
    /* every significand of [1, 2) and [2, 4) */
    for (uint32_t db = 0x3F800000u; db < 0x40800000u; db++) {
        float d = fl(db);
        for (int k = 0; k < 6; k++) { one(numerator(turn), d, turn); turn = (turn + 1) %% BINADES; }
        volatile float vd = d;
        float y = 1.0f / vd;
        volatile float D = d * 0x1p64f, ys = y * 0x1p-64f;
        /* (+0 for a zero of either sign, as div_tail gives it: the clamp behind the divide does not tell the two zeros apart) */
        zero_bad += bits(div_scaled4(0.0f, D, ys)) != 0u || bits(div_scaled4(-0.0f, D, ys)) != 0u || bits(div_tail(-0.0f, d, y)) != 0u;
    }
    /* across [2^-126, 4): divisor exponent fields 1 .. 128, numerators up to 2^34 times the divisor (field e + 34 -> binade e + 56) */
    for (uint32_t i = 0; i < (1u << 14); i++)
        for (uint32_t e = 1; e <= 128; e++) {
            const float d = fl((e << 23) | (rnd() & 0x007FFFFFu));
            const int top = (int)e + 56 < BINADES ? (int)e + 56 : BINADES - 1;
            for (int k = 0; k < 8; k++) { one(numerator((int)(rnd() %% (uint32_t)(top + 1))), d, -1); small_d += e < 127; }
        }
    /* near 2^-126 (exponent field 1: binades 0 .. 57) */
    for (uint32_t i = 0; i < (1u << 16); i++) {
        const float ds[3] = {fl(0x00800000u + i), fl(0x00FFFFFFu - i), fl(0x00800000u + (rnd() & 0x007FFFFFu))};
        for (int j = 0; j < 3; j++)
            for (int b = 0; b < 58; b += 1 + (int)(rnd() %% 3)) one(numerator(b), ds[j], -1);
    }
    /* near 2 and near 2^2 */
    for (uint32_t i = 0; i < (1u << 12); i++) {
        const float ds[4] = {fl(0x40800000u + i), fl(0x40800000u - 1u - i), fl(0x40000000u + i), fl(0x40000000u - 1u - i)};
        for (int j = 0; j < 4; j++)
            for (int b = 0; b < BINADES; b++) one(numerator(b), ds[j], -1);
    }
    unsigned long long least = ~0ull;
    for (int b = 0; b < BINADES; b++) if (per_binade[b] < least) least = per_binade[b];
    printf("%%llu %%llu %%llu %%llu %%llu %%llu %%llu %%llu %%llu %%llu %%08llx %%08llx\n", total, bad, denormal_q, tiny_n, ordinary, tail_differs, scaled_differs, zero_bad, least, small_d,
           first_n, first_d);
    return 0;
}
"""


def _device_function(name):
    """The text of a `__device__ __forceinline__ float name(...) { ... }` of sweep_common.hpp, as it stands."""
    text = open(HPP).read()
    m = re.search(r"^__device__ __forceinline__ float " + name + r"\(.*?^}\n", text, re.S | re.M)
    assert m, name
    return m.group(0)


def test_div_scaled4_is_the_ieee_quotient(tmp_path):
    src = tmp_path / "div_scaled4.c"
    exe = tmp_path / "div_scaled4"
    src.write_text(MAIN % (_device_function("div_tail") + _device_function("div_scaled") + _device_function("div_scaled4")))
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)], text=True).split()
    total, bad, denormal_q, tiny_n, ordinary, tail_differs, scaled_differs, zero_bad, least, small_d = (int(v) for v in out[:10])
    print(f"pairs {total} (at least {least} in each of the 213 binades 2^-149 .. 2^63; {small_d} with a divisor below 1), differences {bad} "
          f"(first n = 0x{out[10]}, d = 0x{out[11]}); denormal quotients {denormal_q}, tiny numerators {tiny_n}; different from div_scaled {scaled_differs}; "
          f"ordinary pairs {ordinary}, of them different from div_tail {tail_differs}; zero numerators wrong {zero_bad}")
    assert total >= 100_000_000 and least >= 450_000 and denormal_q > 5_000_000 and tiny_n > 20_000_000 and small_d > 10_000_000
    assert ordinary > 60_000_000 and tail_differs == 0           # an ordinary numerator: the 3-operation divide's own result
    assert scaled_differs == 0                                    # every pair: the seven-operation form's result
    assert zero_bad == 0
    assert bad == 0
