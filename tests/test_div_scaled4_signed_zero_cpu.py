"""The scaled sweep pair of the from-start tile starts a pixel's weighted sum AT its left term, without the `0 +` in front of it
(csrc/sweep_tile_sweeps.inc wsum, csrc/sweep_common.hpp next to div_scaled4).  The claim: the sum can then be -0 where it was +0 and is
otherwise the same bits, and div_scaled4 answers +0 to both, so every quotient is the same bits.

Nothing is restated here: the body of `wsum` is cut out of sweep_tile_sweeps.inc and div_scaled4 out of sweep_common.hpp, and both are compiled
as C, without contraction (the builtins are the host compiler's too; `constexpr` is defined away, and the switches the text names --
CONTRACT, SCALED, kFromStart -- are variables of the harness: SCALED = 0 is the chain every other sweep keeps, with the `0 +`, SCALED = 1
the lean one).  The arrays the text reads hold one pixel's operands.

Cases, each in both contraction forms, for pixel 0 of a row (whose left term arrives as a finished product from the neighbouring lane)
and for pixel 1 (whose left term is formed in the chain): every combination of four (weight, value) terms out of

  weights   0, 2^-149, 2^-126, 1e-20, 0.5, 1
  values    +0, -0, 2^-149, -2^-149, 1e-30, -1e-30, -2^-140, 100.5, -3.25, 255

which holds left terms and products that are +0 and -0 (a zero weight, a zero value), +-2^-149 (1 * +-2^-149), negative tiny values
whose product underflows to -0 (1e-20 * -1e-30, 2^-149 * -2^-140, 0.5 * -2^-149: a tie that rounds to even) and ordinary values.  The
divisor is the four weights' sum in the kernel's order, 1 where that is 0 (sweep_tile_setup.inc); a denormal divisor belongs to a wave of
the IEEE variant, which never runs this pair, and is left out.  Required: 0 quotients that differ, bit for bit; wherever the two SUMS differ
the one with `0 +` is +0 and the lean one -0; and the cases do hold such sums, so the comparison is not empty."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc")

MAIN = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define __device__
#define __forceinline__ static inline
#define constexpr
%(div)s
enum { G = 3, kFromStart = 1 };
static int CONTRACT, SCALED;
static float cur[G][4], xl0[G], xr3[G], up[4], dn[4], wu0[4], wr[G][4], wd[G][4];
static float wsum(int g, int i) {
%(wsum)s
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static const float W[6] = {0.0f, 0x1p-149f, 0x1p-126f, 1e-20f, 0.5f, 1.0f};
static const float X[10] = {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, 1e-30f, -1e-30f, -0x1p-140f, 100.5f, -3.25f, 255.0f};
int main(void) {
    unsigned long long total = 0, quotient_differs = 0, sum_differs = 0, other_difference = 0, skipped = 0, minus_zero_left = 0, minus_zero_quotient = 0;
    const int g = 1;                                   /* an interior row: its upper and lower neighbours are cur[0] and cur[2] */
    for (CONTRACT = 0; CONTRACT < 2; CONTRACT++)
        for (int i = 0; i < 2; i++)
            for (int a = 0; a < 60; a++) for (int b = 0; b < 60; b++) for (int c = 0; c < 60; c++) for (int e = 0; e < 60; e++) {
                const float wl = W[a %% 6], xl = X[a / 6], wrr = W[b %% 6], xr = X[b / 6], wu = W[c %% 6], xu = X[c / 6], wdn = W[e %% 6], xd = X[e / 6];
                volatile float d0 = 0.0f;
                float d = d0 + wl; d = d + wrr; d = d + wu; d = d + wdn;          /* the divisor, sweep_tile_setup.inc */
                if (d == 0.0f) d = 1.0f;
                if (d < 0x1p-126f) { skipped++; continue; }
                volatile float vd = d;
                const float y = 1.0f / vd;
                volatile float D = d * 0x1p64f, ys = y * 0x1p-64f;
                volatile float left = wl * xl;                               /* pixel 0: the product made in the previous lane */
                if (i == 0) xl0[g] = left; else { wr[g][i - 1] = wl; cur[g][i - 1] = xl; }
                wr[g][i] = wrr; cur[g][i + 1] = xr; wd[g - 1][i] = wu; cur[g - 1][i] = xu; wd[g][i] = wdn; cur[g + 1][i] = xd;
                SCALED = 0; const float with = wsum(g, i);
                SCALED = 1; const float lean = wsum(g, i);
                const float q_with = div_scaled4(with, D, ys), q_lean = div_scaled4(lean, D, ys);
                total++;
                minus_zero_left += bits(left) == 0x80000000u;
                if (bits(with) != bits(lean)) { sum_differs++; other_difference += !(bits(with) == 0u && bits(lean) == 0x80000000u); }
                quotient_differs += bits(q_with) != bits(q_lean);
                minus_zero_quotient += lean == 0.0f && bits(q_lean) != 0u;          /* (a zero sum of either sign; a tiny negative sum may well underflow to -0) */
            }
    printf("%%llu %%llu %%llu %%llu %%llu %%llu %%llu\n", total, quotient_differs, sum_differs, other_difference, skipped, minus_zero_left, minus_zero_quotient);
    return 0;
}
"""


def _div_scaled4():
    text = open(os.path.join(CSRC, "sweep_common.hpp")).read()
    m = re.search(r"^__device__ __forceinline__ float div_scaled4\(.*?^}\n", text, re.S | re.M)
    assert m
    return m.group(0)


def _wsum_body():
    """The statements of `auto wsum = [&](int g, int i) { ... };` in sweep_tile_sweeps.inc, as they stand."""
    text = open(os.path.join(CSRC, "sweep_tile_sweeps.inc")).read()
    m = re.search(r"auto wsum = \[&\]\(int g, int i\) \{\n(.*?)^        \};\n", text, re.S | re.M)
    assert m
    body = m.group(1)
    assert "0.0f + xl0[g]" in body and "return sum;" in body and "SCALED && kFromStart" in body, body      # both chains are in the text that is compiled
    return body


def test_the_sum_chain_without_its_leading_zero_gives_the_same_quotients(tmp_path):
    src = tmp_path / "signed_zero.c"
    exe = tmp_path / "signed_zero"
    src.write_text(MAIN % {"div": _div_scaled4(), "wsum": _wsum_body()})
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"])
    total, quotient_differs, sum_differs, other_difference, skipped, minus_zero_left, minus_zero_quotient = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    print(f"chains {total} (left out for a denormal divisor: {skipped}), a left term of -0 in {minus_zero_left}; sums that differ {sum_differs}, "
          f"of them other than +0 against -0: {other_difference}; quotients that differ {quotient_differs}; zero sums whose quotient is not +0: {minus_zero_quotient}")
    assert total > 40_000_000 and minus_zero_left > 1_000_000
    assert sum_differs > 10_000                 # the `0 +` does matter to the sum: the comparison below is not empty
    assert other_difference == 0                # ... only ever as +0 against -0
    assert minus_zero_quotient == 0             # div_scaled4 gives +0 for a zero numerator of either sign
    assert quotient_differs == 0
