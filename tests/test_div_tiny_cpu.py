"""div_tiny (csrc/sweep_common.hpp): the quotient of a tiny numerator by scaling, restated in C and compared with the IEEE divide.

    N = n * 2^64;  Q = div_tail(N, d, y);  q = Q * 2^-64        y = RN(1/d), d normal and <= 4, 0 < |n| < 2^-100

q is RN(n/d) unless Q lies exactly on a midpoint of the 2^-149 grid (|Q - q * 2^64| == 2^-86) while N/d != Q: those lanes are "suspect" and the
kernels send their row group to the full divide.  A lane whose numerator is not tiny takes a scale of 1: div_tail's quotient, never suspect.
The C restatement uses fmaf and is compiled without contraction, as the kernels' div_tail is written."""
import subprocess

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static float div_tail(float n, float d, float y) { float q0 = n * y; float r = fmaf(-d, q0, n); return fmaf(r, y, q0); }
static float div_tiny(float n, float d, float y, int *suspect, int *rem) {
    int tiny = fabsf(n) < 0x1p-100f;
    float up = tiny ? 0x1p64f : 1.0f, down = tiny ? 0x1p-64f : 1.0f;       /* a lane that is not tiny: div_tail as it stands */
    float N = n * up, Q = div_tail(N, d, y), q = Q * down;
    *suspect = fabsf(fmaf(q, -up, Q)) == 0x1p-86f;
    *rem = fmaf(-d, Q, N) != 0.0f;
    return q;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float fl(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
static unsigned long long total, bad, suspects, suspects_rem, suspects_differ, denormal_q, bad_tie, first_n, first_d;
static void one(float n, float d) {
    if (n == 0.0f) return;                     /* a zero numerator is not tiny: the kernels' test is 0 < |n| < 2^-100 */
    volatile float vn = n, vd = d;
    float want = vn / vd, y = 1.0f / vd;
    int sus, rem;
    float got = div_tiny(n, d, y, &sus, &rem);
    total++;
    if (fabsf(want) < 0x1p-126f && want != 0.0f) denormal_q++;
    if (sus) { suspects++; suspects_rem += rem; suspects_differ += bits(got) != bits(want); if (!rem && bits(got) != bits(want)) bad_tie++; }
    else if (bits(got) != bits(want)) { if (!bad) { first_n = bits(n); first_d = bits(d); } bad++; }
}
static unsigned long long big_total, big_bad;
static void one_big(float n, float d) {        /* not tiny: the scale is 1, the result div_tail's, never suspect */
    volatile float vn = n, vd = d;
    float want = vn / vd, y = 1.0f / vd;
    int sus, rem;
    float got = div_tiny(n, d, y, &sus, &rem);
    big_total++;
    if (sus || bits(got) != bits(want)) big_bad++;
}
int main(void) {
    /* numerators that are NOT tiny, up to 2^100 (times 2^64 they would overflow), in the same row group as tiny ones */
    for (int i = 0; i < 2000000; i++) {
        uint32_t nb = 0x0D800000u + rnd() % (0x71800000u - 0x0D800000u); if (rnd() & 1) nb |= 0x80000000u;
        uint32_t db = 0x35800000u + rnd() % (0x40800000u - 0x35800000u + 1u);
        one_big(fl(nb), fl(db));
    }
    /* seeded: numerators below 2^-100 in every binade down to the denormals, both signs; divisors from 2^-126 to 4 */
    for (int i = 0; i < 6000000; i++) {
        uint32_t nb = rnd() % 0x0D800000u; if (rnd() & 1) nb |= 0x80000000u;
        uint32_t db = 0x00800000u + rnd() % (0x40800000u - 0x00800000u + 1u);
        one(fl(nb), fl(db));
    }
    /* seeded, divisors in [1/4, 4]: where the quotient of a tiny numerator is itself denormal */
    for (int i = 0; i < 6000000; i++) {
        uint32_t nb = rnd() % 0x0D800000u; if (rnd() & 1) nb |= 0x80000000u;
        uint32_t db = 0x3E800000u + rnd() % (0x40800000u - 0x3E800000u + 1u);
        if (i & 1) { nb &= 0xFFFFF000u; db &= 0xFFFF0000u; }           /* few-bit operands */
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
    printf("%llu %llu %llu %llu %llu %llu %llu %08llx %08llx %llu %llu\n", total, bad, suspects, suspects_rem, suspects_differ, denormal_q, bad_tie, first_n, first_d,
           big_total, big_bad);
    return 0;
}
"""


def test_div_tiny_is_the_ieee_quotient_outside_the_suspects(tmp_path):
    src = tmp_path / "div_tiny.c"
    exe = tmp_path / "div_tiny"
    src.write_text(SRC)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)], text=True).split()
    total, bad, suspects, suspects_rem, suspects_differ, denormal_q, bad_tie = (int(v) for v in out[:7])
    print(f"pairs {total}, denormal quotients {denormal_q}, mismatches outside the suspects {bad} (first n = 0x{out[7]}, d = 0x{out[8]}), "
          f"suspects {suspects}, of them with a non-zero remainder {suspects_rem}, really different {suspects_differ}, suspects with a zero remainder that differ {bad_tie}")
    big_total, big_bad = int(out[9]), int(out[10])
    print(f"numerators that are not tiny: {big_total}, suspect or different from the IEEE quotient {big_bad}")
    assert big_total > 1_000_000 and big_bad == 0
    assert total > 10_000_000 and denormal_q > 1_000_000
    assert bad == 0
    assert bad_tie == 0          # with a zero remainder Q IS the quotient, and ties-to-even on it is the IEEE result
    # the guard is exercised: suspects whose remainder is not zero occur, and some of them are in fact wrong without it
    assert suspects_rem > 0 and suspects_differ > 0
    # and it is a guard, not the rule: a suspect needs a denormal quotient
    assert suspects <= denormal_q
