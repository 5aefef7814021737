// lm_views_layout_pins.cpp -- pins the block layout of the views build (csrc/orbx_layout.h: LmViews) beside
// tests/cpp/layout_pins.cpp and tests/cpp/wp_layout_pins.cpp: each `want` is the chain of section sizes written out
// with its align_up_sz, compared with what the header gives over 1 .. 256 windows of 2 .. 8 poses and a set of slot
// capacities around the workgroup size.  Every section starts at a multiple of 256 (a double of the table is never
// split across the alignment the kernels assume) and holds its array.  A mismatch prints the shape; the exit status is
// 1 if there was any.  Host only (tests/test_orbx_lm_abi.py compiles and runs it).
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
  const size_t caps[] = {1, 5, 63, 64, 255, 256, 257, 2000, 65536};
  for (size_t n = 1; n <= 256; n++)
    for (size_t len = 2; len <= 8; len++)
      for (size_t cap : caps) {
        std::snprintf(g_shape, sizeof g_shape, "n=%zu len=%zu cap=%zu", n, len, cap);
        const LmViews V(n, cap, len);
        EQ(V.slots, n * cap);
        EQ(V.table, 0);
        EQ(V.reason, A(8 * 16 * n * len));
        EQ(V.reproj_px, A(8 * 16 * n * len) + A(n * cap));
        EQ(V.bytes, A(8 * 16 * n * len) + A(n * cap) + 4 * n * cap);
      }
  std::printf("%lld values compared, %lld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
