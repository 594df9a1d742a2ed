"""div_tiny (csrc/sweep_common.hpp) in its one-rounding form, restated in C and compared with the host's IEEE divide.

    up = tiny ? 2^64 : 1,  down = tiny ? 2^-64 : 1                  tiny: |n| < 2^-100
    N = n * up;  qd = (N * y) * down;  R = fma(-d, qd * up, N);  q = fma(R, y * down, qd)            y = RN(1/d), d normal and <= 4

qd is a point of the quotient's own grid (the 2^-149 grid where the quotient is denormal) next to n/d, R is the remainder against it,
and the last fma adds the correction and rounds ONCE, to that grid: no midpoint can be met twice, so there are no suspects and no IEEE
divide behind it.  With a scale of 1 the three lines are div_tail as it stands.  Required: 0 differences, over every binade below
2^-100 (the denormals included), numerators that are not tiny, and the pairs that the two-rounding form of tests/test_div_tiny_cpu.py
got wrong (its suspects that really differ: the cases its guard existed for).  Compiled without contraction; a few seconds."""
import subprocess

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static float div_tail(float n, float d, float y) { float q0 = n * y; float r = fmaf(-d, q0, n); return fmaf(r, y, q0); }
static float div_tiny(float n, float d, float y) {
    int tiny = fabsf(n) < 0x1p-100f;
    float up = tiny ? 0x1p64f : 1.0f, down = tiny ? 0x1p-64f : 1.0f;
    float N = n * up;
    float qd = (N * y) * down;
    float R = fmaf(-d, qd * up, N);
    return fmaf(R, y * down, qd);
}
/* the two-rounding form this one replaces: its result, and whether it called the lane suspect */
static float div_tiny_twice(float n, float d, float y, int *suspect) {
    int tiny = fabsf(n) < 0x1p-100f;
    float up = tiny ? 0x1p64f : 1.0f, down = tiny ? 0x1p-64f : 1.0f;
    float N = n * up, Q = div_tail(N, d, y), q = Q * down;
    *suspect = fabsf(fmaf(q, -up, Q)) == 0x1p-86f;
    return q;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float fl(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
static unsigned long long total, bad, denormal_q, guarded, guarded_bad, big_total, big_bad, tail_differs, first_n, first_d, per_binade[128];
static void one(float n, float d) {
    if (n == 0.0f) return;                     /* the kernels' test is 0 < |n| < 2^-100 */
    volatile float vn = n, vd = d;
    float want = vn / vd, y = 1.0f / vd;
    float got = div_tiny(n, d, y);
    int sus;
    float old = div_tiny_twice(n, d, y, &sus);
    total++;
    per_binade[(bits(n) >> 23) & 0xFF]++;
    if (fabsf(want) < 0x1p-126f && want != 0.0f) denormal_q++;
    if (sus && bits(old) != bits(want)) { guarded++; guarded_bad += bits(got) != bits(want); }
    if (bits(got) != bits(want)) { if (!bad) { first_n = bits(n); first_d = bits(d); } bad++; }
}
static void one_big(float n, float d) {        /* not tiny: the scale is 1 and the result is div_tail's, bit for bit */
    volatile float vn = n, vd = d;
    float want = vn / vd, y = 1.0f / vd;
    float got = div_tiny(n, d, y);
    big_total++;
    big_bad += bits(got) != bits(want);
    tail_differs += bits(got) != bits(div_tail(n, d, y));
}
int main(void) {
    /* numerators that are not tiny, 2^-100 .. 2^100, divisors 2^-20 .. 4 */
    for (int i = 0; i < 2000000; i++) {
        uint32_t nb = 0x0D800000u + rnd() % (0x71800000u - 0x0D800000u); if (rnd() & 1) nb |= 0x80000000u;
        uint32_t db = 0x35800000u + rnd() % (0x40800000u - 0x35800000u + 1u);
        one_big(fl(nb), fl(db));
    }
    /* every binade below 2^-100, the denormals (exponent field 0) included, the same number of numerators in each; both signs;
       divisors from 2^-126 to 4, and from 1/4 to 4 where the quotient of a tiny numerator is itself denormal */
    for (uint32_t e = 0; e < 27; e++)
        for (int i = 0; i < 400000; i++) {
            uint32_t nb = (e << 23) | (rnd() & 0x007FFFFFu); if (rnd() & 1) nb |= 0x80000000u;
            uint32_t db = (i & 1) ? 0x3E800000u + rnd() % (0x40800000u - 0x3E800000u + 1u) : 0x00800000u + rnd() % (0x40800000u - 0x00800000u + 1u);
            if ((i & 6) == 6) { nb &= 0xFFFFF000u; db &= 0xFFFF0000u; }           /* few-bit operands */
            one(fl(nb), fl(db));
        }
    /* structured: the exact ties.  d = 2, 3, 4 (and their neighbours), numerators a few units of 2^-149 */
    const float ds[] = {2.0f, 3.0f, 4.0f, 1.0f, 1.5f, 2.5f, 3.5f, 0.5f, 0.75f, 1.25f, 0x1.fffffep1f, 0x1.000002p1f, 0x1.800002p1f};
    for (unsigned k = 0; k < sizeof ds / sizeof *ds; k++)
        for (int m = -4096; m <= 4096; m++) one(ldexpf((float)m, -149), ds[k]);
    /* denormal numerators, every one of the low 2^16, and the largest ones, by generic divisors */
    for (int r = 0; r < 16; r++) {
        float d = fl(0x3F800000u + rnd() % 0x01000000u);
        for (uint32_t m = 1; m < 65536u; m++) { one(fl(m), d); one(fl(0x80000000u | (0x007FFFFFu - m)), d); }
    }
    unsigned long long least = ~0ull;
    for (int e = 0; e < 27; e++) if (per_binade[e] < least) least = per_binade[e];
    printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %08llx %08llx\n", total, bad, denormal_q, guarded, guarded_bad, big_total, big_bad, tail_differs, least, first_n, first_d);
    return 0;
}
"""


def test_one_rounding_div_tiny_is_the_ieee_quotient(tmp_path):
    src = tmp_path / "div_tiny_once.c"
    exe = tmp_path / "div_tiny_once"
    src.write_text(SRC)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)], text=True).split()
    total, bad, denormal_q, guarded, guarded_bad, big_total, big_bad, tail_differs, least = (int(v) for v in out[:9])
    print(f"tiny pairs {total} (at least {least} in each of the 27 binades below 2^-100), denormal quotients {denormal_q}, differences {bad} "
          f"(first n = 0x{out[9]}, d = 0x{out[10]}); pairs the two-rounding form got wrong {guarded}, of them wrong here {guarded_bad}; "
          f"not tiny {big_total}: different from the IEEE quotient {big_bad}, from div_tail {tail_differs}")
    assert total > 10_000_000 and least >= 300_000 and denormal_q > 1_000_000
    assert big_total == 2_000_000 and big_bad == 0 and tail_differs == 0       # scale 1 equals div_tail
    assert guarded > 10_000 and guarded_bad == 0                               # the cases the guard existed for
    assert bad == 0
