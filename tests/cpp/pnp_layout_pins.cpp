// pnp_layout_pins.cpp -- pins the record of the PnP path and its two block layouts (include/orbx_pnp.h:
// orbx_pnp_record; csrc/orbx_internal.h: OrbxPnpRecord, OrbxPnpCorr; csrc/orbx_layout.h: PnpBlock, PnpScratch) beside
// tests/cpp/wp_layout_pins.cpp.  The record's size and offsets are static_asserts and are printed for the ctypes
// structure to be compared with (tests/test_orbx_pnp_abi.py compiles and runs this); each layout `want` is the chain of
// section sizes written out with its align_up_sz, over 1 .. 256 windows of 3 .. 8 frames and five slot counts.
// A mismatch prints the shape; the exit status is 1 if there was any.  Host only.
#include <cstddef>
#include <cstdio>

#include "../../include/orbx_pnp.h"
#include "../../visual-odometry-gpu_amd/csrc/orbx_layout.h"

using namespace orbx_layout;

static_assert(sizeof(orbx_pnp_record) == 72 && alignof(orbx_pnp_record) == 8, "orbx_pnp_record");
static_assert(offsetof(orbx_pnp_record, pose6) == 0 && offsetof(orbx_pnp_record, inliers) == 48 &&
                  offsetof(orbx_pnp_record, iters) == 52 && offsetof(orbx_pnp_record, n_corr) == 56 &&
                  offsetof(orbx_pnp_record, status) == 60 && offsetof(orbx_pnp_record, rms_px) == 64,
              "orbx_pnp_record");
static_assert(sizeof(OrbxPnpRecord) == sizeof(orbx_pnp_record) && offsetof(OrbxPnpRecord, inliers) == 48 &&
                  offsetof(OrbxPnpRecord, iters) == 52 && offsetof(OrbxPnpRecord, n_corr) == 56 &&
                  offsetof(OrbxPnpRecord, status) == 60 && offsetof(OrbxPnpRecord, rms_px) == 64,
              "OrbxPnpRecord");
static_assert(sizeof(OrbxPnpCorr) == 40 && offsetof(OrbxPnpCorr, x) == 24 && offsetof(OrbxPnpCorr, y) == 32,
              "OrbxPnpCorr");
static_assert(sizeof(orbx_window_poses_pnp_view) == 3 * 8 + 3 * 4 + 4, "orbx_window_poses_pnp_view");
static_assert(ORBX_PNP_OK == 0 && ORBX_PNP_SKIPPED == 1 && ORBX_PNP_FEW_POINTS == 2 && ORBX_PNP_NO_MODEL == 3,
              "orbx_pnp_status");

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
  std::printf("record size %zu pose6 %zu inliers %zu iters %zu n_corr %zu status %zu rms_px %zu\n",
              sizeof(orbx_pnp_record), offsetof(orbx_pnp_record, pose6), offsetof(orbx_pnp_record, inliers),
              offsetof(orbx_pnp_record, iters), offsetof(orbx_pnp_record, n_corr), offsetof(orbx_pnp_record, status),
              offsetof(orbx_pnp_record, rms_px));
  std::printf("view size %zu records %zu poses6 %zu mask %zu slot_capacity %zu window_len %zu n_windows %zu\n",
              sizeof(orbx_window_poses_pnp_view), offsetof(orbx_window_poses_pnp_view, records),
              offsetof(orbx_window_poses_pnp_view, poses6), offsetof(orbx_window_poses_pnp_view, mask),
              offsetof(orbx_window_poses_pnp_view, slot_capacity), offsetof(orbx_window_poses_pnp_view, window_len),
              offsetof(orbx_window_poses_pnp_view, n_windows));
  const size_t caps[5] = {1, 8, 65, 200, 4096};
  for (size_t n = 1; n <= 256; n++)
    for (size_t len = 3; len <= 8; len++)
      for (size_t cap : caps) {
        std::snprintf(g_shape, sizeof g_shape, "n=%zu len=%zu cap=%zu", n, len, cap);
        const size_t problems = n * (len - 2);
        const PnpBlock B(n, cap, len);
        EQ(B.problems, problems);
        EQ(B.records, 0);
        EQ(B.poses6, A(72 * problems));
        EQ(B.mask, A(72 * problems) + A(8 * 6 * n * len));
        EQ(B.bytes, A(72 * problems) + A(8 * 6 * n * len) + A(problems * cap));
        const PnpScratch S(n, cap, len);
        EQ(S.corr, 0);
        EQ(S.cidx, A(40 * problems * cap));
        EQ(S.bytes, A(40 * problems * cap) + A(4 * problems * cap));
      }
  std::printf("%lld values compared, %lld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
