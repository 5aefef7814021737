// tile_tables_radius_sweep.cpp -- host-only check of the tables build_tile_tables (csrc/orbx_tables.h) makes for EVERY
// NMS radius the library accepts (nms_window 0 .. 7: R = 0, 1, 2, 3), both FAST kernels, first passes of 0, 1 and 2
// tile rows, default / learned / chosen / forced cuts.  plan_tables_replay.cpp pins the tables' bytes at R = 1; this
// program asserts what the kernels RELY ON, restated here from what they read and independent of the builders'
// own arithmetic:
//   1. the pyramid rows of the first pass reach every row its FAST units (ring 3 rows + NMS window R rows below the
//      unit) and the descriptors of their keypoints (ORBX_TOP_MARGIN - 1 rows below the keypoint) can read; where a
//      level has an early band, the first pass ends at P >= D + R + 3 and >= h0 + ORBX_TOP_MARGIN, and the band's
//      strips -- tested on tile row 0 alone -- cover [P, D + ORBX_TOP_MARGIN);
//   2. first-pass and second-pass strips together cover every row of every strip column exactly once;
//   3. the FAST units of a level tile its rows exactly once, none taller than its kernel holds, first-pass units first;
//   4. the strips / tiles in x and the mask words of a row cover the level's width, each strip's context inside the
//      256 pixels it loads.
// Test infrastructure only; built with -fsanitize=address,undefined by tests/test_cpp_tile_tables_radius.py.
#include <cstdio>
#include <string>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_tables.h"

using namespace orbx_tables;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                           \
  do {                                                             \
    if (!(cond)) {                                                 \
      if (g_fail++ < 30) {                                         \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                                  \
        std::printf("\n");                                         \
      }                                                            \
    }                                                              \
  } while (0)

orbx_params params_for(float scale, int nlevels, int w, int h, int nms_window) {
  orbx_params p{};
  p.nfeatures = 1000;
  p.scale_factor = scale;
  p.nlevels = nlevels;
  p.threshold = 20;
  p.n = 9;
  p.nms_window = nms_window;
  p.patch_size = 31;
  p.harris_window = 7;
  p.harris_k = 0.04f;
  p.select_mode = ORBX_SELECT_HARRIS;
  p.blur_levels = ORBX_BLUR_ALL;
  p.blur_kind = ORBX_BLUR_SEP16;
  p.max_width = w;
  p.max_height = h;
  p.max_batch = 1;
  return p;
}

struct Frame {
  orbx_params p{};
  OrbxPlan plan{};
  std::vector<OrbxResizeTap> taps;
  OrbxTableCapacity cap{};
};
// the most levels, up to `nlevels`, that the library accepts for the size
bool make_frame(int w, int h, float scale, int nlevels, int nms_window, int fast_impl, Frame* F) {
  std::string why;
  for (; nlevels >= 1; nlevels--) {
    F->p = params_for(scale, nlevels, w, h, nms_window);
    OrbxPlan M;
    if (build_plan(F->p, w, h, &M, &why, fast_impl) != ORBX_OK) continue;
    if (table_capacity(F->p, M, fast_impl, 2, &F->cap, &why) != ORBX_OK) continue;
    return plan_with_taps(F->p, w, h, fast_impl, &F->plan, &F->taps, &why) == ORBX_OK;
  }
  return false;
}

struct Counts {
  long long cases = 0, cut_levels = 0, band_levels = 0, two_pass_levels = 0, one_pass_levels = 0, clamped_cuts = 0;
};

struct Case {
  int w, h, R, fast_impl, top;
  float scale;
  const char* state;
};
#define TAG "%d x %d scale %.1f R %d kernel %d top %d %s level %d"
#define TAGV c.w, c.h, (double)c.scale, c.R, c.fast_impl, c.top, c.state, l

// ---- 3. the FAST units ---------------------------------------------------------------------------------------------------
// rows [y0, y0 + rows) of every tile row of level l, as the kernels read them from the units' records
struct TileRow {
  int y0 = -1, rows = 0, units = 0;
};
void check_fast_units(const Case& c, const OrbxPlan& P, const OrbxPlanTables& T, std::vector<std::vector<TileRow>>* rows_of) {
  const OrbxBandMap& bm = T.bm_fast;
  const std::vector<OrbxTileDesc>& U = T.tiles[T_FAST];
  rows_of->assign(P.nlevels, {});
  for (int l = 0; l < P.nlevels; l++) (*rows_of)[l].assign(bm.tiles_y[l], TileRow{});
  CHECK((size_t)bm.band_begin[bm.nbands] == U.size(), "%zu units, band map says %d", U.size(), bm.band_begin[bm.nbands]);
  const int umax = fast_unit_rows_max(c.fast_impl, c.R);
  int prev_ty = 0;
  for (size_t i = 0; i < U.size(); i++) {
    const OrbxTileDesc& d = U[i];
    const int l = d.l;
    CHECK(l >= 0 && l < P.nlevels && d.ty >= 0 && d.ty < bm.tiles_y[l], "unit %zu: level %d tile row %d", i, l, d.ty);
    if (l < 0 || l >= P.nlevels || d.ty < 0 || d.ty >= bm.tiles_y[l]) continue;
    // band-major: the units of the first pass are the first band_begin[top] of the table (enqueue_batch launches them
    // by that count), and a unit's probe looks at tile rows launched before it
    CHECK(d.ty >= prev_ty, "unit %zu: tile row %d after tile row %d", i, d.ty, prev_ty);
    prev_ty = d.ty;
    CHECK(((int)i < bm.band_begin[d.ty + 1]) && ((int)i >= bm.band_begin[d.ty]), "unit %zu of tile row %d outside its band", i, d.ty);
    const int y0 = (int)(d.pad & 0xffffu), rows = (int)(d.pad >> 16);
    TileRow& r = (*rows_of)[l][d.ty];
    if (r.units == 0) r.y0 = y0, r.rows = rows;
    CHECK(r.y0 == y0 && r.rows == rows, TAG ": units of tile row %d disagree on their rows", TAGV, d.ty);
    CHECK(d.tx == r.units, TAG ": tile row %d has unit %d at place %d", TAGV, d.ty, d.tx, r.units);
    r.units++;
    CHECK(rows >= 1 && rows <= umax, TAG ": a unit of %d rows, the kernel holds %d", TAGV, rows, umax);
    CHECK(d.w == P.L[l].w && d.h == P.L[l].h && d.pitch == P.L[l].pitch && d.u0 == P.L[l].cap && d.u1 == P.L[l].mask_wpr &&
              d.u2 == bm.tiles_x[l] && d.img_off == (uint64_t)P.L[l].img_off && d.mask_off == (uint64_t)P.L[l].mask_off &&
              d.stat_index == (uint32_t)(l * ORBX_MAX_BANDS),
          TAG ": a unit's record is not its level's", TAGV);
  }
  for (int l = 0; l < P.nlevels; l++) {
    int y = 0;
    for (int b = 0; b < bm.tiles_y[l]; b++) {
      const TileRow& r = (*rows_of)[l][b];
      CHECK(r.units == bm.tiles_x[l], TAG ": tile row %d has %d of %d units", TAGV, b, r.units, bm.tiles_x[l]);
      CHECK(r.y0 == y, TAG ": tile row %d starts at row %d, the one above ended at %d", TAGV, b, r.y0, y);
      CHECK(r.y0 < P.L[l].h, TAG ": tile row %d starts below the level", TAGV, b);
      y = r.y0 + r.rows;
    }
    CHECK(bm.tiles_y[l] >= 1 && y >= P.L[l].h, TAG ": the tile rows end at row %d of %d", TAGV, y, P.L[l].h);
  }
}

// ---- 4. the level's width ------------------------------------------------------------------------------------------------
void check_width(const Case& c, const OrbxPlan& P, const OrbxBandMap& bm) {
  int mask_off = 0;
  for (int l = 0; l < P.nlevels; l++) {
    const OrbxLevel& L = P.L[l];
    const int n = bm.tiles_x[l], R = c.R;
    CHECK(L.mask_off == mask_off, TAG ": mask block at word %d, the level above ends at %d", TAGV, L.mask_off, mask_off);
    mask_off += L.mask_wpr * L.h;
    if (c.fast_impl == 4) {
      // k_fast4: strip s loads dwords [s S, s S + 64); emits the pixels [P0, P1) of them -- from the strip's first
      // pixel if it is the first strip, to its last if it is the last, its HD halo dwords excluded otherwise --, for
      // which it needs the ring (3 px) and the NMS window (R px) to either side; its mask words hold pixels
      // [mask_strip_px s, + 256)
      const int HD = (R + 3 + 3) / 4, S = 64 - 2 * HD;
      CHECK(4 * HD >= R + 3, "halo of %d dwords for R %d", HD, R);
      CHECK(L.mask_strip_px == 4 * S && L.mask_wpr == 4 * n, TAG ": mask_strip_px %d mask_wpr %d for %d strips of %d lanes", TAGV,
            L.mask_strip_px, L.mask_wpr, n, S);
      int x = 0;
      for (int s = 0; s < n; s++) {
        const int load0 = 4 * s * S, load1 = load0 + 256;
        const int P0 = s == 0 ? 0 : load0 + 4 * HD, P1 = s + 1 == n ? load1 : load1 - 4 * HD;
        CHECK(P0 == x && P1 > P0, TAG ": strip %d emits from pixel %d, the one before ended at %d", TAGV, s, P0, x);
        x = P1;
        // what the strip looks at of the level: inside the dwords it loads
        const int lo = std::max(std::max(P0, 3) - R - 3, 0), hi = std::min(std::min(P1, L.w - 3) + R + 3, L.w);
        CHECK(hi <= lo || (lo >= load0 && hi <= load1), TAG ": strip %d reads pixels [%d, %d), loads [%d, %d)", TAGV, s, lo, hi, load0, load1);
        // ... and inside its own four mask words
        CHECK(P0 >= L.mask_strip_px * s && P1 <= L.mask_strip_px * s + 256, TAG ": strip %d's pixels leave its mask words", TAGV, s);
        CHECK(P0 < L.w || s == 0, TAG ": strip %d starts past the level's width", TAGV, s);
      }
      CHECK(x >= L.w, TAG ": the strips end at pixel %d of %d", TAGV, x, L.w);
    } else {
      CHECK(L.mask_strip_px == 0 && L.mask_wpr * 64 >= L.w && (L.mask_wpr - 1) * 64 < L.w, TAG ": %d mask words for %d px", TAGV, L.mask_wpr, L.w);
      CHECK(n * ORBX_FAST3_TW >= L.w && (n - 1) * ORBX_FAST3_TW < L.w, TAG ": %d tiles for %d px", TAGV, n, L.w);
    }
    CHECK(L.pitch >= L.w && L.pitch % 64 == 0, TAG ": pitch %d", TAGV, L.pitch);
  }
  CHECK(P.mask_words == mask_off, "mask block of %d words, the levels take %d", P.mask_words, mask_off);
}

// ---- 1. and 2. the pyramid strips of the two passes ----------------------------------------------------------------------
// per strip column of level l: how often each row is produced by the strips of `tiles` that `want` accepts
template <class F>
void cover(const std::vector<OrbxTileDesc>& tiles, int l, int ntx, int h, std::vector<std::vector<int>>* n, F want) {
  n->assign(ntx, std::vector<int>(h, 0));
  for (const OrbxTileDesc& d : tiles) {
    if (d.l != l || !want(d)) continue;
    if (d.tx < 0 || d.tx >= ntx || d.ty < 0 || d.f < 1 || d.ty + d.f > h) {
      CHECK(false, "a strip of level %d: column %d of %d, rows [%d, %d) of %d", l, d.tx, ntx, d.ty, d.ty + d.f, h);
      continue;
    }
    for (int y = d.ty; y < d.ty + d.f; y++) (*n)[d.tx][y]++;
  }
}
// every column covers exactly [r0, r1), once
bool is_range(const std::vector<std::vector<int>>& n, int r0, int r1) {
  for (const auto& col : n)
    for (int y = 0; y < (int)col.size(); y++)
      if (col[y] != (y >= r0 && y < r1 ? 1 : 0)) return false;
  return true;
}
int skip_rows(const OrbxTileDesc& d) { return (int)((d.mask_off >> 32) & 0x3fffffffu); }

void check_pyramid_strips(const Case& c, const OrbxPlan& P, const OrbxPlanTables& T, const OrbxAdapt& a,
                          const std::vector<std::vector<TileRow>>& fast_rows, Counts* n) {
  const OrbxBandMap& bm = T.bm_fast;
  const std::vector<OrbxTileDesc>&top = T.tiles[T_PYRBLUR_TOP], &rest = T.tiles[T_PYRBLUR_REST], &whole = T.tiles[T_PYRBLUR];
  const int R = c.R;
  int reporters = 0, top_levels = 0;
  for (int l = 0; l < P.nlevels; l++) {
    const OrbxLevel& L = P.L[l];
    const int h = L.h, ntx = pyrblur_strips_x(L.w);
    // a strip column produces 248 px (62 dwords), one dword more in the first and in the last column
    CHECK(L.w <= 256 ? ntx == 1 : 4 * (62 * ntx + 2) >= L.w, TAG ": %d strip columns for %d px", TAGV, ntx, L.w);
    std::vector<std::vector<int>> first, second, band, both, all;
    // the whole table (one pass): every row once
    cover(whole, l, ntx, h, &all, [](const OrbxTileDesc&) { return true; });
    CHECK(is_range(all, 0, h), TAG ": the one-pass table does not cover every row once", TAGV);
    cover(top, l, ntx, h, &first, [](const OrbxTileDesc&) { return true; });
    cover(rest, l, ntx, h, &second, [](const OrbxTileDesc&) { return true; });
    both = first;
    for (int x = 0; x < ntx; x++)
      for (int y = 0; y < h; y++) both[x][y] += second[x][y];
    CHECK(is_range(both, 0, h), TAG ": the two passes together do not cover every row once", TAGV);  // 2.
    // the first pass is a prefix [0, E) of the rows, the same in every column
    int E = 0;
    while (E < h && first[0][E]) E++;
    CHECK(is_range(first, 0, E), TAG ": the first pass is not the rows [0, %d) in every column", TAGV, E);
    for (const OrbxTileDesc& d : top)
      if (d.l == l) CHECK((int)d.pad == ntx && d.u0 == L.xtab_off && d.u1 == L.ytab_off && d.u2 == L.win8 && d.w == L.w && d.h == h && d.pitch == L.pitch && d.img_off == (uint64_t)L.img_off, TAG ": a first-pass strip's record is not its level's", TAGV);
    const bool two = c.top > 0 && bm.tiles_y[l] > c.top;
    if (!two) {
      // no second pass for the level: no FAST unit of it is launched after the second pyramid pass that could wait for it
      CHECK(E == h, TAG ": one FAST launch, but the first pyramid pass ends at row %d of %d", TAGV, E, h);
      n->one_pass_levels++;
      continue;
    }
    n->two_pass_levels++;
    // D: the end of the first-pass FAST tile rows, from the units' own records
    const TileRow& last = fast_rows[l][c.top - 1];
    const int D = last.y0 + last.rows;
    const int fast_reads = std::min(h, D + R + 3);            // ring + NMS window below the last row of a unit
    const int late = std::min(h, D + ORBX_TOP_MARGIN);       // + what the descriptors of keypoints in rows < D read
    CHECK(ORBX_TOP_MARGIN >= R + 3, "margin %d for R %d", ORBX_TOP_MARGIN, R);
    const int h0 = bm.first_h[l][0];
    if (h0 > 0) {
      n->cut_levels++;
      CHECK(c.top == 2 && fast_rows[l][0].rows == h0 && fast_rows[l][1].y0 == h0 && h0 + bm.first_h[l][1] == D &&
                D == 2 * bm.tile_h[l],
            TAG ": cut %d + %d, first pass of %d rows", TAGV, h0, bm.first_h[l][1], D);
    }
    CHECK(E == a.early_rows[l] || (E == h && a.early_rows[l] >= h), TAG ": the first pass ends at %d, the record says %d", TAGV, E, a.early_rows[l]);
    CHECK(E >= fast_reads, TAG ": the first pyramid pass ends at row %d, its FAST units read to %d (D = %d)", TAGV, E, fast_reads, D);
    if (E < late) {
      // an early band: only under an uneven cut; the frames that filled in tile row 0 have their keypoints above h0
      n->band_levels++;
      CHECK(h0 > 0, TAG ": the first pass ends at %d < %d without a cut", TAGV, E, late);
      CHECK(E >= std::min(h, h0 + ORBX_TOP_MARGIN), TAG ": the first pass ends at %d, descriptors above the cut %d read to %d", TAGV, E, h0, h0 + ORBX_TOP_MARGIN);
      cover(rest, l, ntx, h, &band, [&](const OrbxTileDesc& d) { return d.ty < late; });
      CHECK(is_range(band, E, late), TAG ": the band's strips do not cover [%d, %d)", TAGV, E, late);
    }
    if (late < h) top_levels++;
    for (const OrbxTileDesc& d : rest) {
      if (d.l != l) continue;
      const bool in_band = d.ty < late;
      CHECK(in_band ? d.ty + d.f <= late : true, TAG ": a strip crosses the end of the band", TAGV);
      // the band is skipped on tile row 0's verdict alone, the rest on the whole first pass's
      CHECK(skip_rows(d) == (in_band ? 1 : std::min(c.top, bm.tiles_y[l])), TAG ": a second-pass strip at row %d tests %d tile rows", TAGV, d.ty, skip_rows(d));
      CHECK((uint32_t)d.mask_off == (uint32_t)L.cap && d.stat_index == (uint32_t)(l * ORBX_MAX_BANDS) && (int)d.pad == ntx, TAG ": a second-pass strip's record is not its level's", TAGV);
      if (d.mask_off >> 62 & 1) {
        reporters++;
        CHECK(!in_band, TAG ": the reporting strip is a band's", TAGV);
      }
    }
  }
  CHECK(reporters == (rest.empty() ? 0 : 1), "%d reporting strips among %zu second-pass strips", reporters, rest.size());
  CHECK(T.top_levels.n == top_levels, "%d levels with a second pass, top_levels lists %d", top_levels, T.top_levels.n);
}

// ---- the scheduler states -----------------------------------------------------------------------------------------------
struct State {
  const char* name;
  bool pipeline;
  void (*set)(OrbxAdapt& a);
};
void learned_rows(OrbxAdapt& a) {
  const int rows[] = {33, 28, 40, 20, 16, 0, 24, 17};
  for (int l = 0; l < 8; l++) a.tile_h_pref[l] = rows[l];
}
void chosen_cut(OrbxAdapt& a) {
  a.tile_h_pref[0] = a.tile_h_pref[1] = 40;
  a.cut_pref[0] = 61;
  a.cut_pref[1] = 54;
}
void band_pays(OrbxAdapt& a) {
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.fill_last[l][fill_bucket(8)] += 900, a.fill_last[l][fill_bucket(120)] += 100;
}
const State kStates[] = {
    {"fresh", true, [](OrbxAdapt&) {}},
    {"pipeline off", false, [](OrbxAdapt& a) { learned_rows(a); }},
    {"learned rows", true, [](OrbxAdapt& a) { learned_rows(a); }},
    {"chosen cut, band pays", true, [](OrbxAdapt& a) { chosen_cut(a), band_pays(a); }},
    {"chosen cut, no histogram", true, [](OrbxAdapt& a) { chosen_cut(a); }},
    // forced cuts (the nearest cut the kernel can run is taken): shorter than R + 3, a group, mid-way, the last row
    {"forced 1", true, [](OrbxAdapt& a) { first_split_fields(a, "2:1,1,1,1,1,1,1,1,1,1,1,1"); }},
    {"forced 4", true, [](OrbxAdapt& a) { first_split_fields(a, "2:4,4,4,4,4,4,4,4,4,4,4,4"); }},
    {"forced 7", true, [](OrbxAdapt& a) { first_split_fields(a, "2:7,7,7,7,7,7,7,7,7,7,7,7"); }},
    {"forced 20", true, [](OrbxAdapt& a) { first_split_fields(a, "2:20,20,20,20,20,20,20,20,20,20,20,20"); }},
    {"forced 33", true, [](OrbxAdapt& a) { first_split_fields(a, "2:33,31,29,27,25,23,21,19"); }},
    {"forced 47", true, [](OrbxAdapt& a) { first_split_fields(a, "2:47,46,45,44,43,42,41,40"); }},
    {"forced 61", true, [](OrbxAdapt& a) { first_split_fields(a, "2:61,60,59,58,57,56,55,54"); }},
    {"forced 80", true, [](OrbxAdapt& a) { first_split_fields(a, "2:80,79,78,77,76,75,74,73"); }},
    {"forced 97", true, [](OrbxAdapt& a) { first_split_fields(a, "2:97,95,93,91,89,87,85,83"); }},
    {"forced 500", true, [](OrbxAdapt& a) { first_split_fields(a, "2:500,500,500,500,500,500,500,500"); }},
    {"forced over learned rows", true, [](OrbxAdapt& a) { learned_rows(a), first_split_fields(a, "2:30,9,55,12,9,0,3,20"); }},
    {"forced, late", true, [](OrbxAdapt& a) { first_split_fields(a, "2:late:20,20,20,20,20,20,20,20"); }},
    {"equal", true, [](OrbxAdapt& a) { chosen_cut(a), first_split_fields(a, "2:equal:20,20,20,20"); }},
};

void sweep_size(int w, int h, int nlevels, Counts* n) {
  OrbxPlanTables T;
  for (float scale : {1.2f, 1.5f, 2.0f})
    for (int nms_window : {0, 3, 5, 7})
      for (int fast_impl : {4, 3}) {
        Frame F;
        const bool ok = make_frame(w, h, scale, nlevels, nms_window, fast_impl, &F);
        CHECK(ok, "%d x %d at scale %.1f, nms_window %d: no plan", w, h, (double)scale, nms_window);
        if (!ok) continue;
        const int R = nms_window / 2;
        for (int top = 0; top <= 2; top++)
          for (const State& s : kStates) {
            const Case c{w, h, R, fast_impl, top, scale, s.name};
            OrbxAdapt a;
            s.set(a);
            const OrbxTableSwitches sw{fast_impl, 2, top, true, s.pipeline && top > 0};
            std::string why;
            const int st = build_tile_tables(F.plan, R, sw, F.cap, a, nullptr, &T, &why);
            CHECK(st == ORBX_OK, "%d x %d scale %.1f R %d kernel %d top %d %s: %s", w, h, (double)scale, R, fast_impl, top, s.name, why.c_str());
            if (st != ORBX_OK) continue;
            n->cases++;
            std::vector<std::vector<TileRow>> fast_rows;
            check_fast_units(c, F.plan, T, &fast_rows);
            check_width(c, F.plan, T.bm_fast);
            check_pyramid_strips(c, F.plan, T, a, fast_rows, n);
            // a forced cut the kernel cannot run went to one it can
            for (int l = 0; l < F.plan.nlevels; l++)
              if (a.cut_force[l] > 0 && T.bm_fast.first_h[l][0] > 0 && T.bm_fast.first_h[l][0] != a.cut_force[l]) n->clamped_cuts++;
          }
      }
}

}  // namespace

int main() {
  const struct {
    int w, h, nlevels;
  } sizes[] = {{1241, 376, 8}, {1920, 1080, 8}, {160, 160, 12}, {645, 487, 8}, {27, 27, 8}, {320, 160, 4}};
  Counts n;
  for (const auto& s : sizes) {
    const long long before = n.cases;
    sweep_size(s.w, s.h, s.nlevels, &n);
    std::printf("%d x %d: %lld cases\n", s.w, s.h, n.cases - before);
  }
  std::printf("%lld cases: levels with two passes %lld, with one %lld, with a cut %lld (%lld moved to a legal one), with an early band %lld\n",
              n.cases, n.two_pass_levels, n.one_pass_levels, n.cut_levels, n.clamped_cuts, n.band_levels);
  CHECK(n.two_pass_levels > 0 && n.one_pass_levels > 0 && n.cut_levels > 0 && n.clamped_cuts > 0 && n.band_levels > 0,
        "a kind of level the sweep never met");
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
