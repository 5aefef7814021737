"""harris_fast<K> (the packed 16-bit Harris window of k_level_select / k_lvl_harris) against harris_at on the HOST:
the two functions are cut out of csrc/orbx_kernels.hip as they stand and compiled with g++, with the three GPU
operations they use restated in C (v_alignbyte_b32, v_perm_b32 with selectors 0..7 and 0x0c, packed 16-bit add / sub
that wrap per half).  Every position harris_fast_ok admits, on frames whose width covers every byte alignment of a
row's end, with noise and with 0/1/254/255 frames (Sobel sums of +-1020, ties): the responses must agree bit for bit.
Needs no GPU; what it cannot see is the compiler's GPU code, which the GPU tests cover."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
using std::max;
using std::min;
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline int reflect101(int i, int n) { if (i < 0) i = -i; if (i >= n) i = 2 * n - 2 - i; return i; }
static inline uint32_t emu_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3)));
}
static inline uint32_t emu_perm(uint32_t a, uint32_t b, uint32_t sel) {  // bytes 0..3 of {a:b} are b's
  const uint64_t v = (((uint64_t)a) << 32) | b;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t s = (sel >> (8 * i)) & 0xff;
    if (s >= 8 && s != 0x0c) abort();  // no other selector is used
    r |= (s < 8 ? (uint32_t)((v >> (8 * s)) & 0xff) : 0u) << (8 * i);
  }
  return r;
}
static inline uint32_t pk_add(uint32_t a, uint32_t b) { return ((a + b) & 0xffffu) | ((((a >> 16) + (b >> 16)) & 0xffffu) << 16); }
static inline uint32_t pk_sub(uint32_t a, uint32_t b) { return ((a - b) & 0xffffu) | ((((a >> 16) - (b >> 16)) & 0xffffu) << 16); }
"""

MAIN = r"""
template <int K>
long run(int w, int h, int pitch, unsigned seed, int kind) {
  std::vector<uint8_t> img((size_t)pitch * h + 16);  // the pool's tail slack: the last row's third dword
  srand(seed);
  for (auto& p : img) {
    const int r = rand();
    p = kind == 0 ? (uint8_t)(r & 255) : (uint8_t)(((r >> 3) & 1 ? 254 : 0) + (r & 1));
  }
  float g[K * K];
  for (int i = 0; i < K * K; i++) g[i] = (float)(1 + rand() % 97) / 531.0f;
  long bad = 0, n = 0;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      if (!harris_fast_ok(w, h, x, y, K)) continue;
      const float a = harris_at(img.data(), w, h, pitch, x, y, g, K, 0.04f);
      const float b = harris_fast<K>(img.data(), w, h, pitch, x, y, g, 0.04f);
      n++;
      if (memcmp(&a, &b, 4)) {
        if (bad++ < 5) printf("K=%d %dx%d (%d, %d): %a vs %a\n", K, w, h, x, y, a, b);
      }
    }
  printf("K=%d %dx%d pitch %d kind %d: %ld positions, %ld differ\n", K, w, h, pitch, kind, n, bad);
  return n > 0 ? bad : 1;
}
int main() {
  long bad = 0;
  for (int kind = 0; kind < 2; kind++)
    for (int w = 16; w <= 23; w++) {
      const int pitch = w == 20 ? 32 : (w + 3) & ~3;
      bad += run<7>(w, 13, pitch, w * 7 + kind, kind) + run<5>(w, 11, pitch, w * 5 + kind, kind) +
             run<3>(w, 9, pitch, w * 3 + kind, kind);
    }
  bad += run<3>(4, 4, 4, 1, 1);  // the smallest frame harris_fast_ok admits: both columns / rows reflect
  printf("differ in all: %ld\n", bad);
  return bad != 0;
}
"""


def test_packed_harris_equals_harris_at_on_the_host(tmp_path):
    src = open(os.path.join(ROOT, "visual-odometry-gpu_amd", "csrc", "orbx_kernels.hip")).read()
    a = src.index("__device__ __forceinline__ float harris_at(")
    b = src.index("__device__ __forceinline__ float harris_any(")
    body = src[a:b].replace("__builtin_amdgcn_", "emu_").replace("__device__ __forceinline__", "static inline")
    body = body.replace("__restrict__", "")
    assert "harris_fast(" in body and "harris_fast_ok(" in body
    cpp, exe = str(tmp_path / "harris_host.cpp"), str(tmp_path / "harris_host")
    with open(cpp, "w") as f:
        f.write(PRE + body + MAIN)
    # -ffp-contract=off as in csrc/Makefile; the sanitizers check the window's loads against the frame's buffer
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, cpp], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
