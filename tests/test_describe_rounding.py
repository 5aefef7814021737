"""The interior path of k_describe2 rounds each rotated BRIEF coordinate with
orbx_lround_small (csrc/orbx_math.h): the truncation of v + copysign(0.5 - 2^-25, v)
instead of the multi-step lroundf restatement.  This compiles the header for the
HOST with gcc and checks it EXHAUSTIVELY against this machine's lroundf: every
float with |v| < 32 (the rotated pattern points lie within 13 * sqrt(2) px), both
signs, zeros, subnormals and every half-way value n + 0.5 included.  The helper is
a bit insert, one IEEE add (round to nearest) and a truncating convert; gfx950 does
the same operations, so the GPU gets the same integers (tests/test_gpu_parity.py).
"""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <math.h>
#include <stdio.h>
#include "%s/visual-odometry-gpu_amd/csrc/orbx_math.h"
int main(void){
  const uint32_t top = orbx_f2u(32.0f);  /* exclusive: every float with |v| < 32 */
  long n = 0, halves = 0, bad = 0;
  for (uint32_t u = 0; u < top; u++) for (uint32_t sg = 0; sg < 2; sg++) {
    const float v = orbx_u2f(u | (sg << 31));
    n++;
    if (v - truncf(v) == (sg ? -0.5f : 0.5f)) halves++;
    if (lroundf(v) != (long)orbx_lround_small(v)) bad++;
  }
  printf("%%ld %%ld %%ld\n", n, halves, bad);
  return 0;
}
"""


def test_lround_small_matches_lroundf_for_every_float_below_32():
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "r.c")
        with open(c, "w") as fh:
            fh.write(SRC % ROOT)
        exe = os.path.join(d, "r")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", c, "-o", exe, "-lm"])
        out = subprocess.check_output([exe], timeout=600).decode().split()
    n, halves, bad = map(int, out)
    assert n == 2 * 0x42000000  # 2.2e9 values
    assert halves == 2 * 32  # 0.5, 1.5, ..., 31.5 and their negatives
    assert bad == 0
