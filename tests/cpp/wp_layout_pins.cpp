// wp_layout_pins.cpp -- pins the three block layouts of the window-poses path (csrc/orbx_layout.h: WpInput, WpBlock,
// WbBlock) beside tests/cpp/layout_pins.cpp: each `want` is the chain of section sizes written out with its
// align_up_sz, compared with what the header gives over 1 .. 1024 windows of 2 .. 8 frames.  Every section starts at a
// multiple of 256 (a double is never split across the alignment the kernels assume) and holds its array.  A mismatch
// prints the shape; the exit status is 1 if there was any.  Host only (tests/test_orbx_vo_abi.py compiles and runs it).
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
  for (size_t n = 1; n <= 1024; n++) {
    std::snprintf(g_shape, sizeof g_shape, "n=%zu", n);
    const WpInput I(n);
    EQ(I.T0, 0);
    EQ(I.scale0, A(8 * 16 * n));
    EQ(I.bytes, A(8 * 16 * n) + 8 * n);
    for (size_t len = 2; len <= 8; len++) {
      std::snprintf(g_shape, sizeof g_shape, "n=%zu len=%zu", n, len);
      const WpBlock B(n, len);
      EQ(B.poses6, 0);
      EQ(B.poses4x4, A(8 * 6 * n * len));
      EQ(B.status, A(8 * 6 * n * len) + A(8 * 16 * n * len));
      EQ(B.bytes, A(8 * 6 * n * len) + A(8 * 16 * n * len) + A(4 * n));
      const WbBlock W(n, len);
      EQ(W.poses4x4, 0);
      EQ(W.updated, A(8 * 16 * n * len));
      EQ(W.bytes, A(8 * 16 * n * len) + A(n * len));
    }
  }
  std::printf("%lld values compared, %lld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
