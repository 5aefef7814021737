// st_layout_pins.cpp -- pins the block layouts of the stitch (csrc/orbx_layout.h: StInput, StBlock) beside
// tests/cpp/layout_pins.cpp and tests/cpp/lm_views_layout_pins.cpp: each `want` is the chain of section sizes written
// out with its align_up_sz, compared with what the header gives over 1 .. 256 windows of 2 .. 8 frames and every
// stride a window length allows.  Every section starts at a multiple of 256 and holds its array.  A mismatch prints
// the shape; the exit status is 1 if there was any.  Host only (tests/test_orbx_stream_abi.py compiles and runs it).
#include <cstdio>

#include "../../visual-odometry-gpu_amd/csrc/orbx_layout.h"

using namespace orbx_layout;

namespace {

long long g_checks = 0, g_failures = 0;
char g_shape[64];

void check(const char* what, size_t got, size_t want) {
  g_checks++;
  if (got == want) return;
  if (++g_failures <= 50) std::printf("FAIL %s: %s = %zu, want %zu\n", g_shape, what, got, want);
}
#define EQ(got, want) check(#got, (size_t)(got), (size_t)(want))

size_t A(size_t v) { return align_up_sz(v, 256); }

}  // namespace

int main() {
  for (size_t n = 1; n <= 256; n++)
    for (size_t len = 2; len <= 8; len++)
      for (size_t stride = 1; stride <= len - 1; stride++) {
        std::snprintf(g_shape, sizeof g_shape, "n=%zu len=%zu stride=%zu", n, len, stride);
        const size_t F = (n - 1) * stride + len;
        const StInput I(n);
        EQ(I.T_start, 0);
        EQ(I.links, 256);
        EQ(I.broken, 256 + A(8 * 14 * n));
        EQ(I.bytes, 256 + A(8 * 14 * n) + 4 * n);
        const StBlock B(n, len, stride);
        EQ(B.frames, F);
        EQ(st_stream_frames(n, len, stride), F);
        EQ(B.trajectory4x4, 0);
        EQ(B.owner, A(8 * 16 * F));
        EQ(B.anchors4x4, A(8 * 16 * F) + A(4 * F));
        EQ(B.lambda, A(8 * 16 * F) + A(4 * F) + A(8 * 16 * n));
        EQ(B.status, A(8 * 16 * F) + A(4 * F) + A(8 * 16 * n) + A(8 * n));
        EQ(B.bytes, A(8 * 16 * F) + A(4 * F) + A(8 * 16 * n) + A(8 * n) + A(4 * n));
      }
  std::printf("%lld values compared, %lld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
