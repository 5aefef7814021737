// pyramid_early_band_sweep.cpp -- host-only checks of the early band of the fused pyramid + blur kernel's second pass
// (csrc/orbx_plan.h: pyrblur_early_rows, build_pyrblur_tiles with early_rows, pyrblur_early_strips_bound,
// early_band_pays): the rows between h0 + ORBX_TOP_MARGIN and the end of the first pass, produced in the second
// pass unless tile row 0 alone holds the cap.  Calls the code the library itself runs; the tables without the new
// argument are compared with a restatement of the builder as it was before the band existed.  Test infrastructure
// only; built with -fsanitize=address,undefined by tests/test_cpp_pyramid_early_band.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_plan.h"

using namespace orbx_geom;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail++ < 12) {                                \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

OrbxPlan plan_of(int nlevels, const int* w, const int* h) {
  OrbxPlan P;
  std::memset(&P, 0, sizeof(P));
  P.nlevels = nlevels;
  P.w0 = w[0];
  P.h0 = h[0];
  for (int l = 0; l < nlevels; l++) {
    P.L[l].w = w[l];
    P.L[l].h = h[l];
    P.L[l].pitch = align_up(w[l], 64);
    P.L[l].cap = 100 + l;
    P.L[l].win8 = l == 1 ? 1 : 0;
    P.L[l].img_off = l * 4096 * 64;
  }
  return P;
}

// the builder before the early band: part 0 every row, part 1 rows [0, split), part 2 rows [split, h)
size_t old_build(const OrbxPlan& plan, int max_rows, std::vector<OrbxTileDesc>* out, bool heavy_first, int part,
                 const OrbxBandMap* bm, int top_rows) {
  out->clear();
  bool have_reporter = false;
  for (int l = 0; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    const int dw = (L.w + 3) / 4;
    const int ntx = dw <= 64 ? 1 : (dw - 2 + 61) / 62;
    const int split = part == 0 ? L.h : pyrblur_first_pass_rows(plan, *bm, l, top_rows);
    const int r0 = part == 2 ? split : 0, r1 = part == 1 ? split : L.h;
    if (r1 <= r0) continue;
    const int nb = (r1 - r0 + max_rows - 1) / max_rows, rows = (r1 - r0 + nb - 1) / nb;
    for (int b = 0; b < nb; b++)
      for (int tx = 0; tx < ntx; tx++) {
        OrbxTileDesc d{};
        d.l = l;
        d.tx = tx;
        d.ty = r0 + b * rows;
        d.f = std::min(rows, r1 - d.ty);
        d.w = L.w;
        d.h = L.h;
        d.pitch = L.pitch;
        d.u0 = L.xtab_off;
        d.u1 = L.ytab_off;
        d.u2 = L.win8;
        d.pad = (uint32_t)ntx;
        d.img_off = (uint64_t)L.img_off;
        if (part == 2) {
          d.stat_index = (uint32_t)(l * ORBX_MAX_BANDS);
          d.mask_off = ((uint64_t)(uint32_t)std::min(top_rows, bm->tiles_y[l]) << 32) | (uint32_t)L.cap;
          if (b == 0 && tx == 0 && !have_reporter) {
            d.mask_off |= 1ull << 62;
            have_reporter = true;
          }
        }
        if (d.f > 0) out->push_back(d);
      }
  }
  if (heavy_first) {
    auto cost = [](const OrbxTileDesc& d) { return (d.f + 4) * (d.l == 0 ? 35 : d.u2 == 1 ? 80 : 90); };
    std::stable_sort(out->begin(), out->end(), [&](const OrbxTileDesc& a, const OrbxTileDesc& b) { return cost(a) > cost(b); });
  }
  return out->size();
}

bool same_tables(const std::vector<OrbxTileDesc>& a, const std::vector<OrbxTileDesc>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(OrbxTileDesc)));
}

long long g_bands = 0;

// one band map: the boundary, the three row ranges, the strips' skip fields, the pool bound, the old tables
void check_tables(const OrbxPlan& P, const OrbxPlan& M, const OrbxBandMap& bm, int R) {
  const int top = 2;
  std::vector<OrbxTileDesc> t1, t2, o;
  int early[ORBX_MAX_LEVELS] = {};
  for (int l = 0; l < P.nlevels; l++) early[l] = pyrblur_early_rows(P, bm, l, top, R);
  // without the argument, with zeros and with the late boundary itself: today's tables, entry for entry
  int zeros[ORBX_MAX_LEVELS] = {}, lates[ORBX_MAX_LEVELS] = {};
  for (int l = 0; l < P.nlevels; l++) lates[l] = pyrblur_first_pass_rows(P, bm, l, top);
  for (int heavy = 0; heavy <= 1; heavy++)
    for (int part = 0; part <= 2; part++) {
      old_build(P, ORBX_PYRBLUR_RH, &o, heavy != 0, part, &bm, top);
      const size_t n = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t1, heavy != 0, part, &bm, top);
      CHECK(n == o.size() && same_tables(t1, o), "part %d heavy %d: the table without early_rows changed", part, heavy);
      build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t1, heavy != 0, part, &bm, top, zeros);
      CHECK(same_tables(t1, o), "part %d heavy %d: early_rows = 0 changed the table", part, heavy);
      build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t1, heavy != 0, part, &bm, top, lates);
      CHECK(same_tables(t1, o), "part %d heavy %d: early_rows = late changed the table", part, heavy);
      CHECK(build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, nullptr, heavy != 0, part, &bm, top, early) ==
                build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t1, heavy != 0, part, &bm, top, early),
            "count-only call disagrees");
    }
  const size_t n1 = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t1, false, 1, &bm, top, early);
  const size_t n2 = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, &t2, true, 2, &bm, top, early);
  // the pool: the bound next to the builder, for this size and within a larger maximum's
  const size_t whole = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, nullptr), wholeM = build_pyrblur_tiles(M, ORBX_PYRBLUR_RH, nullptr);
  CHECK(n1 <= whole && n2 <= whole + pyrblur_early_strips_bound(P), "h %d: %zu / %zu strips, whole %zu + %zu", P.L[0].h, n1, n2,
        whole, pyrblur_early_strips_bound(P));
  CHECK(n1 <= wholeM && n2 <= wholeM + pyrblur_early_strips_bound(M), "h %d: the maximum's pool", P.L[0].h);
  int reporters = 0;
  for (int l = 0; l < P.nlevels; l++) {
    const int h = P.L[l].h, nx = pyrblur_strips_x(P.L[l].w), late = lates[l], E = early[l];
    const bool cut = bm.first_h[l][0] > 0 && bm.tiles_y[l] > top && late < h;
    CHECK(E <= late && E >= 1, "level %d: early %d late %d", l, E, late);
    if (!cut) CHECK(E == late, "level %d: a band without a cut (early %d late %d)", l, E, late);
    if (cut) {
      const int h0 = bm.first_h[l][0], D = h0 + bm.first_h[l][1];
      CHECK(late == std::min(h, D + ORBX_TOP_MARGIN), "level %d: the late boundary moved: %d", l, late);
      // descriptors of keypoints of tile row 0 reach row h0 - 1 + 20; the FAST units of tile rows 0 and 1 read up to
      // row D - 1 + R + 3
      CHECK(E >= std::min(h, h0 + ORBX_TOP_MARGIN), "level %d: first pass ends at %d, h0 %d", l, E, h0);
      CHECK(E >= std::min(h, D + R + 3), "level %d: first pass ends at %d, FAST reads to %d", l, E, D + R + 3);
      CHECK(E == std::min(late, std::max(h0 + ORBX_TOP_MARGIN, D + R + 3)), "level %d: boundary %d", l, E);
      if (E < late) g_bands++;
    }
    // rows of the three ranges: [0, E) first pass, [E, late) band, [late, h) rest -- each exactly once per strip column
    std::vector<int> seen((size_t)h * nx, 0);
    for (const OrbxTileDesc& d : t1) {
      if (d.l != l) continue;
      CHECK(d.ty >= 0 && d.ty + d.f <= E && d.f >= 1 && d.f <= ORBX_PYRBLUR_RH && d.mask_off == 0, "level %d: first-pass strip %d+%d", l, d.ty, d.f);
      for (int y = d.ty; y < d.ty + d.f; y++) seen[(size_t)y * nx + d.tx]++;
    }
    for (const OrbxTileDesc& d : t2) {
      if (d.l != l) continue;
      const int na = (int)((d.mask_off >> 32) & 0xffu);
      const bool band = d.ty < late;
      CHECK(d.f >= 1 && d.f <= ORBX_PYRBLUR_RH && d.ty + d.f <= h, "level %d: strip %d+%d", l, d.ty, d.f);
      CHECK((uint32_t)d.mask_off == (uint32_t)P.L[l].cap && d.stat_index == (uint32_t)(l * ORBX_MAX_BANDS), "level %d: skip fields", l);
      if (band) {
        CHECK(d.ty >= E && d.ty + d.f <= late, "level %d: band strip %d+%d outside [%d, %d)", l, d.ty, d.f, E, late);
        CHECK(na == 1 && !(d.mask_off >> 62), "level %d: band strip na %d reporter %d", l, na, (int)(d.mask_off >> 62));
      } else {
        CHECK(na == std::min(top, bm.tiles_y[l]) && na == 2, "level %d: rest strip na %d", l, na);
        reporters += (int)((d.mask_off >> 62) & 1);
      }
      CHECK(d.w == P.L[l].w && d.h == h && d.pitch == P.L[l].pitch && d.pad == (uint32_t)nx && d.img_off == (uint64_t)P.L[l].img_off &&
                d.u2 == (uint32_t)P.L[l].win8, "level %d: level fields", l);
      for (int y = d.ty; y < d.ty + d.f; y++) seen[(size_t)y * nx + d.tx]++;
    }
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1, "level %d (h %d): row %zu covered %d times", l, h, i / nx, seen[i]);
  }
  CHECK(reporters == (n2 && [&] { for (const OrbxTileDesc& d : t2) if (d.ty >= lates[d.l]) return true; return false; }() ? 1 : 0),
        "%d reporters", reporters);
}

void sweep() {
  long long cases = 0;
  const int wM[2] = {300, 250}, hM[2] = {400, 333};
  const OrbxPlan M = plan_of(2, wM, hM);
  for (int strips = 0; strips <= 1; strips++)
    for (int R = 1; R <= 3; R += 2) {
      const int unit_max = strips ? ORBX_FAST_UNIT_ROWS_MAX : orbx_fast3_tile_h(R);
      for (int h = 8; h <= 400; h++) {
        const int w[2] = {300, 250}, hh[2] = {h, std::max(8, h * 5 / 6)};
        const OrbxPlan P = plan_of(2, w, hh);
        const int prefs[4] = {0, ORBX_MIN_TILE_H, 29, 40};
        for (int pi = 0; pi < 4; pi++) {
          int pref[ORBX_MAX_LEVELS] = {};
          pref[0] = pref[1] = prefs[pi];
          OrbxBandMap bm0;
          std::string why;
          if (make_bandmap(P, R, &bm0, &why, strips != 0, pi ? pref : nullptr) != ORBX_OK) continue;
          check_tables(P, M, bm0, R);  // equal halves: no band anywhere
          const int D = 2 * bm0.tile_h[0], D1 = 2 * bm0.tile_h[1];
          for (int a = 1; a < D; a++) {  // every legal pair (h0, D) of the level's depth
            if (!(bm0.tiles_y[0] >= 2 && a < h && a <= unit_max && D - a <= unit_max)) continue;
            int first[ORBX_MAX_LEVELS][2] = {};
            first[0][0] = a;
            first[0][1] = D - a;
            // (and a cut on the second level, where one is legal)
            const int a1 = std::min(std::max(a * D1 / D, 1), D1 - 1);
            if (bm0.tiles_y[1] >= 2 && a1 < hh[1] && a1 <= unit_max && D1 - a1 <= unit_max) first[1][0] = a1, first[1][1] = D1 - a1;
            OrbxBandMap bm;
            if (make_bandmap(P, R, &bm, &why, strips != 0, pi ? pref : nullptr, first) != ORBX_OK) continue;
            CHECK(bm.first_h[0][0] == a, "the pair was not applied");
            check_tables(P, M, bm, R);
            cases++;
          }
        }
      }
    }
  std::printf("tables: %lld (level height, preference, pair) cases, %lld levels with a band\n", cases, g_bands);
}

void hist_add(uint32_t* hist, int fill_row, uint32_t n) { hist[fill_bucket(fill_row)] += n; }

void check_rule() {
  uint32_t hist[ORBX_FILL_BUCKETS] = {};
  const int h0 = 68;
  // an empty histogram: nothing is known
  CHECK(!early_band_pays(hist, h0, 11, 35) && !early_band_pays(hist, h0, 20, 90), "empty histogram");
  // all frames leave: the rows saved against one exit of 100 -- 11 rows of level 0 (385), 3 rows of a gathered
  // level (270), not 3 rows of level 0 (105 against a dearer exit, 90 against the library's)
  hist_add(hist, 60, 1000);
  CHECK(ORBX_PYRBLUR_SKIP_EXIT == 100, "the hand-made cases below were worked out for an exit of 100");
  CHECK(early_band_pays(hist, h0, 11, 35), "all leave, 11 rows x 35");
  CHECK(early_band_pays(hist, h0, 3, 90), "all leave, 3 rows x 90");
  CHECK(early_band_pays(hist, h0, 3, 35) && !early_band_pays(hist, h0, 3, 35, 110) && !early_band_pays(hist, h0, 3, 30), "all leave, 3 rows x 35");
  // ... a band of a row or two never
  CHECK(!early_band_pays(hist, h0, 1, 90) && !early_band_pays(hist, h0, 2, 90) && !early_band_pays(hist, h0, 2, 90, 0), "one-row band");
  CHECK(!early_band_pays(hist, h0, 0, 90) && !early_band_pays(hist, h0, -3, 90), "no band");
  // none leave: every frame pays the warm-up rows
  std::memset(hist, 0, sizeof(hist));
  hist_add(hist, 75, 1000);
  hist_add(hist, 376, 24);
  CHECK(!early_band_pays(hist, h0, 11, 35) && !early_band_pays(hist, h0, 20, 90), "none leave");
  // shares between: 60 of 100 leave, 8 rows x 80: 38400 > 40 x 320 + 60 x 100 = 18800; 30 of 100: 19200 < 25400
  std::memset(hist, 0, sizeof(hist));
  hist_add(hist, 50, 60);
  hist_add(hist, 90, 40);
  CHECK(early_band_pays(hist, h0, 8, 80), "60 %% leave");
  std::memset(hist, 0, sizeof(hist));
  hist_add(hist, 50, 30);
  hist_add(hist, 90, 70);
  CHECK(!early_band_pays(hist, h0, 8, 80), "30 %% leave");
  // the same q as the FAST chooser's: a frame counts as gone only if its whole bucket lies within tile row 0
  std::memset(hist, 0, sizeof(hist));
  hist_add(hist, h0 - 1, 1000);  // rows 65 ... 68 share a bucket that ends at the cut: counted
  CHECK(early_band_pays(hist, h0, 11, 35), "bucket ending at the cut");
  CHECK(!early_band_pays(hist, h0 - 1, 11, 35), "bucket across the cut");
  // the level costs the builder sorts by
  CHECK(pyrblur_row_cost(0, 0) == 35 && pyrblur_row_cost(0, 1) == 35 && pyrblur_row_cost(1, 1) == 80 && pyrblur_row_cost(3, 0) == 90, "row costs");
}

}  // namespace

int main() {
  sweep();
  check_rule();
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
