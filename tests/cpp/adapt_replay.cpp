// adapt_replay.cpp -- host-only replay of the scheduler of the batched path's first pass (csrc/orbx_adapt.h): the
// observation windows, the tile-row heights, the cut of the first pass, the early bands, the adaptive verdict, the
// reset on a new frame size and the parser of ORBX_TOP_ROWS' fields.  Scripted streams assert the value every rule
// gives; a seeded stream per geometry folds every step into a hash whose expected value was recorded from the code
// as it stood BEFORE these rules moved into the header (inside orbx_api.cpp), so the move itself is pinned.  Calls the
// code the library itself runs, and rebuilds the tables after a re-tile with the builder set_plan calls
// (csrc/orbx_tables.h: build_tile_tables), in pools sized by table_capacity for the stream's own frame size.  Test
// infrastructure only; built with -fsanitize=address,undefined by tests/test_cpp_adapt.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

// ---- the scheduler under test -----------------------------------------------------------------------------------------
#include "../../visual-odometry-gpu_amd/csrc/orbx_tables.h"

using namespace orbx_tables;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail++ < 20) {                                \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

// a context as far as the scheduler sees it: the plan and the tables of one frame size, the record, the feedback words
struct Sched {
  orbx_params p{};
  int fast_impl = 4, top = 2;
  bool prefs_on = true;  // what tile_prefs_apply answers: adaptive mode, fused kernel, early exit on
  OrbxPlan plan{};
  OrbxTableCapacity cap{};
  OrbxPlanTables tables;
  OrbxBandMap& bm = tables.bm_fast;
  OrbxAdapt a{};
  uint32_t words[ORBX_FEEDBACK_WORDS] = {};
  long long serial = 0;
  FILE* trace = nullptr;

  int R() const { return p.nms_window / 2; }
  OrbxAdaptGeom geom() const { return OrbxAdaptGeom{plan, bm, R(), fast_impl, top}; }

  // orbx_create and the first batch: the fields of ORBX_TOP_ROWS, the plan, the tables
  void create(int w, int h, int nlevels, int impl, const char* top_rows_value) {
    p.nfeatures = 500;
    p.scale_factor = 1.2f;
    p.nlevels = nlevels;
    p.nms_window = 3;
    p.select_mode = ORBX_SELECT_HARRIS;
    p.blur_levels = ORBX_BLUR_ALL;
    p.blur_kind = ORBX_BLUR_SEP16;
    fast_impl = impl;
    first_split_fields(a, top_rows_value);
    std::string why;
    const int st = build_plan(p, w, h, &plan, &why, fast_impl);
    CHECK(st == ORBX_OK, "build_plan: %s", why.c_str());
    CHECK(table_capacity(p, plan, fast_impl, 2, &cap, &why) == ORBX_OK, "table_capacity: %s", why.c_str());
    new_frame_size(a, w, h, words);
    rebuild();
  }
  // what set_plan does with the record
  void rebuild() {
    std::string why;
    const OrbxTableSwitches sw{fast_impl, 2, top, true, prefs_on};
    const int st = build_tile_tables(plan, R(), sw, cap, a, trace, &tables, &why);
    CHECK(st == ORBX_OK, "build_tile_tables: %s", why.c_str());
  }
  // one batch: the observation step on the words as they stand, and the tables rebuilt if it says so
  bool step() {
    const bool retile = adapt_tile_rows(a, geom(), words, prefs_on, serial, trace);
    if (retile) rebuild();
    serial++;
    return retile;
  }
  void verdict(uint32_t skipped, uint32_t produced) { top_rows_update(a, (uint64_t)produced << 32 | skipped); }
  bool wanted(int top_rows) const { return top_rows_wanted(a, top_rows); }
  void frame_size(int w, int h) { new_frame_size(a, w, h, words); }
};
// ---- end of the scheduler under test ----------------------------------------------------------------------------------

void clear_words(Sched& S) {
  for (int i = 2; i < ORBX_FEEDBACK_WORDS; i++) S.words[i] = 0;
}
// level l reports `need` rows and n frames that filled in row `fill_row`
void report(Sched& S, int l, uint32_t need, int fill_row = 0, uint32_t n = 0) {
  S.words[2 + l] = need;
  if (n) S.words[ORBX_FEEDBACK_HIST + l * ORBX_FILL_BUCKETS + fill_bucket(fill_row)] += n;
}
// steps to the end of the current observation window; true if its last step asked for a re-tile
bool run_window(Sched& S) {
  bool retile = false;
  int guard = 0;
  do {
    retile = S.step();
    CHECK(++guard <= 64, "a window of more than 64 batches");
  } while (S.a.need_batches != 0 && guard <= 64);
  return retile;
}

const int W1 = 1241, H1 = 376, NL1 = 8;    // every level has several tile rows
const int W2 = 160, H2 = 160, NL2 = 12;    // the upper levels have one: tiles_y < 2, lh <= depth

// ---- observation windows -----------------------------------------------------------------------------------------------
void check_windows() {
  Sched S;
  S.create(W1, H1, NL1, 4, "2");
  CHECK(S.plan.L[0].h == 376 && S.bm.tile_h[0] == 47 && S.bm.tiles_y[0] == 8, "level 0: %d rows, tile rows of %d", S.plan.L[0].h, S.bm.tile_h[0]);
  CHECK(S.bm.tiles_y[NL1 - 1] >= 2, "every level of the first geometry has several tile rows");
  report(S, 0, 60);
  // under steady words the windows end after 2, 4, 8, 16, 32, 32 batches
  const int ends[] = {2, 6, 14, 30, 62, 94, 126};
  const int window_after[] = {4, 8, 16, 32, 32, 32, 32};
  int next = 0;
  for (int batch = 1; batch <= 126; batch++) {
    if (batch == 40) report(S, 0, 100);  // mid-window: the first pass has become too short
    const bool retile = S.step();
    const bool end = batch == ends[next];
    CHECK((S.a.need_batches == 0) == end, "batch %d: %d batches into a window", batch, S.a.need_batches);
    if (end) CHECK(S.a.need_window == window_after[next], "batch %d: next window %d", batch, S.a.need_window);
    // decisions fall at the ends of windows only: 60 rows -> 66 with the margin -> tile rows of 33 at the first end;
    // 100 rows -> the default rows again at the end of the window the report fell in
    CHECK(retile == (batch == 2 || batch == 62), "batch %d: re-tile %d", batch, (int)retile);
    if (batch == 2) CHECK(S.a.tile_h_pref[0] == 33 && S.bm.tile_h[0] == 33 && S.a.retiles == 1, "tile rows %d", S.a.tile_h_pref[0]);
    if (batch == 61) CHECK(S.a.tile_h_pref[0] == 33, "no decision inside a window");
    if (batch == 62) CHECK(S.a.tile_h_pref[0] == 0 && S.bm.tile_h[0] == 47 && S.a.retiles == 2, "tile rows %d", S.a.tile_h_pref[0]);
    if (end) next++;
  }
  // a batch whose words are all zero advances no window, not even as the window's last
  Sched Z;
  Z.create(W1, H1, NL1, 4, "2");
  report(Z, 0, 60);
  CHECK(!Z.step() && Z.a.need_batches == 1, "first batch");
  clear_words(Z);
  for (int i = 0; i < 5; i++) CHECK(!Z.step() && Z.a.need_batches == 1 && Z.a.need_window == 2, "an empty batch counted");
  report(Z, 0, 60);
  CHECK(Z.step() && Z.a.need_batches == 0 && Z.a.need_window == 4 && Z.a.tile_h_pref[0] == 33, "the window's second batch");
  // the pipeline cannot run at all (tile_prefs_apply): nothing is observed
  Z.prefs_on = false;
  CHECK(!Z.step() && Z.a.need_batches == 0 && Z.a.need_cur[0] == 0, "observed without the pipeline");
}

// ---- grow at once, shrink for three rows, settle -------------------------------------------------------------------------
void check_heights() {
  Sched S;
  S.create(W1, H1, NL1, 4, "2");
  report(S, 0, 60);
  CHECK(run_window(S) && S.bm.tile_h[0] == 33, "33 rows");
  // grow: 70 rows > 2 x 33 -- at once, although the re-tiles have settled (77 rows with the margin -> 39)
  S.a.retiles = 5;
  clear_words(S);
  report(S, 0, 70);
  CHECK(S.a.need_window == 4 && run_window(S), "grow waits");
  CHECK(S.a.tile_h_pref[0] == 39 && S.bm.tile_h[0] == 39 && S.a.retiles == 6 && S.a.need_window == 8, "grown to %d", S.a.tile_h_pref[0]);
  // shrink: 68 rows -> 37, two rows gained: nothing (both windows the maximum is taken over report 68)
  S.a.retiles = 0;
  clear_words(S);
  report(S, 0, 68);
  CHECK(!run_window(S) && !run_window(S) && S.a.tile_h_pref[0] == 39 && S.a.retiles == 0, "two rows re-tiled");
  CHECK(S.a.need_prev[0] == 68 && S.a.need_window == 32, "windows");
  // 66 rows -> 36, three rows gained: re-tile (the first window still sees the 68 of the one before)
  clear_words(S);
  report(S, 0, 66);
  CHECK(!run_window(S) && S.a.tile_h_pref[0] == 39, "the maximum of two windows");
  CHECK(run_window(S) && S.a.tile_h_pref[0] == 36 && S.bm.tile_h[0] == 36 && S.a.retiles == 1, "three rows: %d", S.a.tile_h_pref[0]);
  // settled (four re-tiles) and the windows still growing: a shrink waits, until the windows have 32 batches
  clear_words(S);
  report(S, 0, 50);
  S.a.retiles = 4;
  S.a.need_window = 8;
  S.a.need_batches = 0;
  S.a.need_prev[0] = 0;
  CHECK(!run_window(S) && S.a.tile_h_pref[0] == 36 && S.a.retiles == 4 && S.a.need_window == 16, "a shrink did not wait");
  CHECK(run_window(S) && S.a.need_window == 32 && S.a.retiles == 5, "a shrink waited on");
  CHECK(S.a.tile_h_pref[0] == 28 && S.bm.tile_h[0] == 28, "50 rows -> 55 -> %d", S.a.tile_h_pref[0]);
  // a level that neither must grow nor gains three rows keeps its height when another level makes the tables change
  clear_words(S);
  report(S, 0, 48);  // 52 rows -> 26: two rows
  report(S, 1, 60);  // default -> 33
  S.a.need_prev[0] = 0;
  CHECK(run_window(S) && S.a.tile_h_pref[0] == 28 && S.a.tile_h_pref[1] == 33, "levels %d %d", S.a.tile_h_pref[0], S.a.tile_h_pref[1]);
  // a report beyond the level counts as the level; a level that needs it all takes the default rows
  clear_words(S);
  report(S, 0, 100000);
  CHECK(run_window(S) && S.a.need_prev[0] == 376 && S.a.tile_h_pref[0] == 0 && S.bm.tile_h[0] == 47, "whole level: %d", S.a.tile_h_pref[0]);
}

// ---- whole groups of 7 rows for the streaming kernel ---------------------------------------------------------------------
void check_group_rounding() {
  // need -> tile rows of level 0, streaming kernel (4) and LDS tile kernel (3)
  const struct { uint32_t need; int h4, h3; } cases[] = {
      {74, 40, 41},  // 81 rows -> 41, one row into a group: 2 x 40 >= 74 + 3
      {76, 40, 42},  // 83 -> 42, two rows into a group: 2 x 40 >= 79
      {77, 40, 42},  // 84 -> 42: 2 x 40 >= 80, the last need that rounds
      {78, 43, 43},  // 85 -> 43, three rows into a group: kept
      {36, 20, 20},  // 40 -> 20, one row into a group, but 2 x 19 < 36 + 3: the margin is used up
      {60, 33, 33},  // 66 -> 33, a whole number of groups
  };
  for (const auto& c : cases)
    for (int impl = 3; impl <= 4; impl++) {
      Sched S;
      S.create(W1, H1, NL1, impl, "2");
      report(S, 0, c.need);
      const int want = impl == 4 ? c.h4 : c.h3;
      CHECK(run_window(S) && S.a.tile_h_pref[0] == want && S.bm.tile_h[0] == want, "need %u, kernel %d: %d rows", c.need, impl, S.a.tile_h_pref[0]);
    }
}

// one window of steady words for level 0: `need` rows, frames by fill row
struct Fill { int row; uint32_t n; };
void level0(Sched& S, uint32_t need, Fill f0, Fill f1 = Fill{0, 0}) {
  clear_words(S);
  report(S, 0, need, f0.row, f0.n);
  if (f1.n) report(S, 0, need, f1.row, f1.n);
}

// ---- where the first pass is cut -----------------------------------------------------------------------------------------
void check_cut() {
  Sched S;
  S.create(W1, H1, NL1, 4, "2");
  // 74 rows -> tile rows of 40, a first pass of 80.  900 of 1000 frames fill by row 60: tile row 0 of 61 rows (9
  // groups) and 100 frames going on through 19 rows: 10200 + (100 x 4200 + 900 x 280) / 1000 = 10872 milli-groups,
  // against 2 x 7200 for equal halves
  level0(S, 74, {60, 900}, {74, 100});
  CHECK(run_window(S) && S.a.tile_h_pref[0] == 40 && S.a.cut_pref[0] == 61, "cut %d of %d", S.a.cut_pref[0], 2 * S.a.tile_h_pref[0]);
  CHECK(S.bm.first_h[0][0] == 61 && S.bm.first_h[0][1] == 19 && S.a.retiles == 1, "pair %d/%d", S.bm.first_h[0][0], S.bm.first_h[0][1]);
  CHECK(S.a.cut_pref[1] == 0 && S.bm.first_h[1][0] == 0, "a level without a histogram was cut");
  // a better cut moves it only for 1000 milli-groups: 800 frames by row 52, 200 by row 60 -- 54 rows would cost
  // 9200 + (200 x 5200 + 800 x 280) / 1000 = 10464 against 10200 + 280: 16 gained, nothing moves
  level0(S, 74, {52, 800}, {60, 200});
  CHECK(!run_window(S) && !run_window(S) && S.a.cut_pref[0] == 61 && S.bm.first_h[0][0] == 61 && S.a.retiles == 1, "moved for 16: %d", S.a.cut_pref[0]);
  // every frame by row 52: 9200 + 280 against 10200 + 280, 1000 gained (the window that still holds the old shares
  // does not move it yet)
  level0(S, 74, {52, 1000});
  CHECK(!run_window(S) && S.a.cut_pref[0] == 61, "moved early");
  CHECK(run_window(S) && S.a.cut_pref[0] == 54 && S.bm.first_h[0][0] == 54 && S.bm.first_h[0][1] == 26 && S.a.retiles == 2, "1000 gained: %d", S.a.cut_pref[0]);
  // new tile-row heights void the cut in force: 900 by row 52, 100 by row 60, with 61 rows in force, gain 508 at a
  // depth of 80 and move nothing; when the level grows to the default rows (90 rows needed -> a first pass of 94),
  // the cut is chosen afresh for that depth: 54 rows at 10172 against 61 at 10480
  Sched V;
  V.create(W1, H1, NL1, 4, "2");
  level0(V, 74, {60, 900}, {74, 100});
  CHECK(run_window(V) && V.a.cut_pref[0] == 61, "cut %d", V.a.cut_pref[0]);
  level0(V, 74, {52, 900}, {60, 100});
  CHECK(!run_window(V) && !run_window(V) && V.a.cut_pref[0] == 61 && V.bm.first_h[0][0] == 61, "moved for 508: %d", V.a.cut_pref[0]);
  level0(V, 90, {52, 900}, {60, 100});
  CHECK(run_window(V) && V.a.tile_h_pref[0] == 0 && V.bm.tile_h[0] == 47, "grown to %d", V.bm.tile_h[0]);
  CHECK(V.a.cut_pref[0] == 54 && V.bm.first_h[0][0] == 54 && V.bm.first_h[0][1] == 40, "cut afresh: %d/%d", V.bm.first_h[0][0], V.bm.first_h[0][1]);
  // a cut that has stopped paying is withdrawn, whatever the gain: 47 rows in force (every frame fills by row 44);
  // then 900 frames by row 36 -- they leave at equal halves too -- and 100 that never fill in the first pass: equal
  // halves cost 8172, the cut 9072, and no other cut beats the halves
  Sched W;
  W.create(W1, H1, NL1, 4, "2");
  level0(W, 74, {44, 1000});
  CHECK(run_window(W) && W.a.cut_pref[0] == 47 && W.bm.first_h[0][0] == 47 && W.bm.first_h[0][1] == 33, "cut %d", W.a.cut_pref[0]);
  level0(W, 74, {36, 900}, {78, 100});
  CHECK(!run_window(W) && W.a.cut_pref[0] == 47, "withdrawn early");
  CHECK(run_window(W) && W.a.cut_pref[0] == 0 && W.bm.first_h[0][0] == 0 && W.a.retiles == 2, "not withdrawn: %d", W.a.cut_pref[0]);
  // equal halves asked for, or the LDS tile kernel: no cut is ever chosen
  for (int k = 0; k < 2; k++) {
    Sched E;
    E.create(W1, H1, NL1, k ? 3 : 4, k ? "2" : "2:equal");
    level0(E, 74, {60, 900}, {74, 100});
    CHECK(run_window(E) && E.a.cut_pref[0] == 0 && E.bm.first_h[0][0] == 0, "cut %d", E.a.cut_pref[0]);
    CHECK(E.a.fill_last[0][fill_bucket(60)] == 1800, "the histogram is kept for the early bands all the same");
  }
}

// ---- forced cuts ---------------------------------------------------------------------------------------------------------
void check_forced() {
  // a forced level is left to its cut, the others to the chooser
  Sched S;
  S.create(W1, H1, NL1, 4, "2:68,65,0,61");
  CHECK(S.bm.first_h[0][0] == 68 && S.bm.first_h[0][1] == 26 && S.bm.first_h[1][0] == 65 && S.bm.first_h[2][0] == 0 && S.bm.first_h[3][0] == 61, "forced pairs");
  clear_words(S);
  for (int l = 0; l < 4; l++) {
    report(S, l, 90, 46, 1000);  // (the default rows stay; every frame fills by row 46, below equal halves)
  }
  CHECK(run_window(S), "level 2 not cut");
  CHECK(S.a.cut_pref[0] == 0 && S.a.cut_pref[1] == 0 && S.a.cut_pref[3] == 0 && S.a.cut_pref[2] == 54, "cuts %d %d %d %d", S.a.cut_pref[0], S.a.cut_pref[1], S.a.cut_pref[2], S.a.cut_pref[3]);
  CHECK(S.bm.first_h[0][0] == 68 && S.bm.first_h[1][0] == 65 && S.bm.first_h[2][0] == 54 && S.bm.first_h[3][0] == 61, "pairs after the re-tile");
  // a forced cut goes to the nearest one the kernel can run: at most unit_max rows and one row less than the first
  // pass or the level, at least depth - unit_max
  Sched hi;
  hi.create(W1, H1, NL1, 4, "2:70000,1");  // streaming kernel, units of up to 128 rows: first passes of 94 and 90
  CHECK(hi.a.cut_force[0] == 65535 && hi.bm.first_h[0][0] == 93 && hi.bm.first_h[0][1] == 1, "upper end: %d/%d", hi.bm.first_h[0][0], hi.bm.first_h[0][1]);
  CHECK(hi.bm.first_h[1][0] == 1 && hi.bm.first_h[1][1] == 89, "lower end: %d/%d", hi.bm.first_h[1][0], hi.bm.first_h[1][1]);
  Sched lo;
  lo.create(W1, H1, NL1, 3, "2:5,5,70000");  // LDS tile kernel, units of up to 47 rows: first passes of 94, 90, 88
  CHECK(lo.bm.first_h[0][0] == 47 && lo.bm.first_h[0][1] == 47, "94 - 47: %d/%d", lo.bm.first_h[0][0], lo.bm.first_h[0][1]);
  CHECK(lo.bm.first_h[1][0] == 43 && lo.bm.first_h[1][1] == 47, "90 - 47: %d/%d", lo.bm.first_h[1][0], lo.bm.first_h[1][1]);
  CHECK(lo.bm.first_h[2][0] == 47 && lo.bm.first_h[2][1] == 41, "unit_max: %d/%d", lo.bm.first_h[2][0], lo.bm.first_h[2][1]);
  // second geometry: level 3 has 93 rows in two tile rows of 47 -- the level is shorter than its first pass; the
  // levels with one tile row take no cut
  Sched sm;
  sm.create(W2, H2, NL2, 4, "2:0,0,0,200,0,0,0,30,30");
  CHECK(sm.plan.L[3].h == 93 && sm.bm.tiles_y[3] == 2 && sm.bm.tile_h[3] == 47, "level 3: %d rows", sm.plan.L[3].h);
  CHECK(sm.bm.first_h[3][0] == 92 && sm.bm.first_h[3][1] == 2, "level height - 1: %d/%d", sm.bm.first_h[3][0], sm.bm.first_h[3][1]);
  CHECK(sm.bm.tiles_y[7] == 1 && sm.bm.tiles_y[8] == 1 && sm.bm.first_h[7][0] == 0 && sm.bm.first_h[8][0] == 0, "one tile row cut");
  // the same without the top-rows-first pipeline: no pair at all
  Sched off;
  off.prefs_on = false;
  off.create(W1, H1, NL1, 4, "2:68");
  CHECK(off.bm.first_h[0][0] == 0 && !off.a.prefs_applied, "cut without the pipeline");
}

// ---- early bands ---------------------------------------------------------------------------------------------------------
void check_early_bands() {
  // chooser: 61 of 80 rows in force, the first pass ends at 101; the rows from max(61 + 21, 80 + 1 + 3) = 84 on are
  // a band of 17 rows that 900 of 1000 frames never need: split
  Sched S;
  S.create(W1, H1, NL1, 4, "2");
  for (int l = 0; l < NL1; l++) CHECK(S.a.early_rows[l] == pyrblur_first_pass_rows(S.plan, S.bm, l, 2), "no cut, no band");
  CHECK(S.a.early_rows[0] == 94 + ORBX_TOP_MARGIN, "default first pass ends at %d", S.a.early_rows[0]);
  level0(S, 74, {60, 900}, {74, 100});
  CHECK(run_window(S) && S.bm.first_h[0][0] == 61 && S.a.early_rows[0] == 84, "band from %d", S.a.early_rows[0]);
  CHECK(S.a.early_rows[1] == 90 + ORBX_TOP_MARGIN, "level 1 ends at %d", S.a.early_rows[1]);
  // 75 of 80 rows: 600 frames by row 72, 400 never (12200 + 1048 = 13248 against 14400: the cut pays); the band has
  // 5 rows, and 600 x 5 x 35 < 400 x 4 x 35 + 600 x 100: kept
  Sched K;
  K.create(W1, H1, NL1, 4, "2");
  level0(K, 74, {72, 600}, {78, 400});
  CHECK(run_window(K) && K.bm.first_h[0][0] == 75 && K.bm.first_h[0][1] == 5, "cut %d", K.bm.first_h[0][0]);
  CHECK(K.a.early_rows[0] == 101, "a band of 5 rows that does not pay must be kept (first pass to 101): ends at %d", K.a.early_rows[0]);
  // forced cuts, no histogram: split from three rows up.  68 of 94: band [98, 115); 87 of 90: [108, 111), three
  // rows; 86 of 88: two rows, kept
  Sched F;
  F.create(W1, H1, NL1, 4, "2:68,87,86");
  CHECK(F.a.early_rows[0] == 98 && F.a.early_rows[1] == 108 && F.a.early_rows[2] == 109, "forced: %d %d %d", F.a.early_rows[0], F.a.early_rows[1], F.a.early_rows[2]);
  // `late`: no band is made, forced or chosen
  Sched L;
  L.create(W1, H1, NL1, 4, "2:late:68,87,86");
  CHECK(L.bm.first_h[0][0] == 68 && L.a.early_rows[0] == 115 && L.a.early_rows[1] == 111, "late: %d %d", L.a.early_rows[0], L.a.early_rows[1]);
  Sched L2;
  L2.create(W1, H1, NL1, 4, "2:late");
  level0(L2, 74, {60, 900}, {74, 100});
  CHECK(run_window(L2) && L2.bm.first_h[0][0] == 61 && L2.a.early_rows[0] == 101, "late, chosen cut: %d", L2.a.early_rows[0]);
  // levels without a second pass end at their height
  Sched sm;
  sm.create(W2, H2, NL2, 4, "2");
  for (int l = 0; l < NL2; l++)
    if (sm.bm.tiles_y[l] <= 2) CHECK(sm.a.early_rows[l] == sm.plan.L[l].h, "level %d ends at %d", l, sm.a.early_rows[l]);
  CHECK(sm.a.early_rows[NL2] == 0, "rows of a level the plan does not have");
}

// ---- the second geometry's short levels ------------------------------------------------------------------------------------
void check_short_levels() {
  Sched S;
  S.create(W2, H2, NL2, 4, "2");
  CHECK(S.plan.L[0].h == 160 && S.bm.tiles_y[0] == 4 && S.bm.tile_h[0] == 40, "level 0: %d tile rows of %d", S.bm.tiles_y[0], S.bm.tile_h[0]);
  CHECK(S.plan.L[7].h == 45 && S.bm.tiles_y[7] == 1 && S.plan.L[11].h == 22, "levels 7, 11: %d, %d rows", S.plan.L[7].h, S.plan.L[11].h);
  // level 7 (45 rows, one tile row of 45): 20 rows -> 24 -> tile rows of 12 asked for (make_bandmap gives 23: never
  // more tile rows than the level above, which has 2); every frame fills by row 8, and a first pass of 46 rows is
  // longer than the level: no cut
  clear_words(S);
  report(S, 7, 20, 8, 1000);
  CHECK(run_window(S) && S.a.tile_h_pref[7] == 12 && S.bm.tile_h[7] == 23 && S.bm.tiles_y[7] == 2, "level 7: %d asked, %d got", S.a.tile_h_pref[7], S.bm.tile_h[7]);
  CHECK(S.a.cut_pref[7] == 0, "one tile row cut at %d", S.a.cut_pref[7]);
  CHECK(!run_window(S) && !run_window(S) && S.a.cut_pref[7] == 0 && S.a.retiles == 1, "a level no longer than its first pass cut at %d", S.a.cut_pref[7]);
  // level 0: 30 rows -> 34 -> 17; a first pass of 34 rows, every frame by row 12: tile row 0 of 12 rows
  clear_words(S);
  report(S, 0, 30, 12, 1000);
  CHECK(run_window(S) && S.a.retiles == 2, "level 0 kept");
  CHECK(S.a.tile_h_pref[0] == 17 && S.bm.tile_h[0] == 17 && S.a.cut_pref[0] == 12 && S.bm.first_h[0][0] == 12 && S.bm.first_h[0][1] == 22, "level 0: %d rows, cut %d", S.a.tile_h_pref[0], S.a.cut_pref[0]);
}

// ---- the adaptive verdict ------------------------------------------------------------------------------------------------
void check_verdict() {
  Sched S;
  S.create(W1, H1, NL1, 4, "2");
  CHECK(S.a.top_on && S.wanted(2) && !S.wanted(0), "starts on");
  S.verdict(2, 6);  // exactly a quarter skipped: stays on
  CHECK(S.a.top_on && S.a.feedback_seen[0] == 2 && S.a.feedback_seen[1] == 6, "a quarter");
  S.verdict(3, 15);  // 1 of 10: off, and this batch is the first one-pass batch
  CHECK(!S.a.top_on && !S.wanted(2) && S.a.top_single_batches == 1, "under a quarter: on %d, %d batches", (int)S.a.top_on, S.a.top_single_batches);
  for (int i = 2; i <= 127; i++) {
    S.verdict(3, 15);  // nothing new arrives in one pass
    CHECK(!S.a.top_on && S.a.top_single_batches == i, "batch %d: %d", i, S.a.top_single_batches);
  }
  S.verdict(3, 15);  // the 128th probes
  CHECK(S.a.top_on && S.a.top_single_batches == 0 && S.wanted(2), "no probe");
  S.verdict(3, 25);  // the probe skipped nothing: off again, counted from one
  CHECK(!S.a.top_on && S.a.top_single_batches == 1, "probe failed");
  S.verdict(13, 26);  // late words of a batch that did skip: on
  CHECK(S.a.top_on, "back on");
  // running totals that wrap past 2^32 give the right deltas
  S.verdict(0xfffffff0u, 0xfffffff8u);
  CHECK(S.a.feedback_seen[0] == 0xfffffff0u && S.a.feedback_seen[1] == 0xfffffff8u, "seen");
  S.verdict(0x00000010u, 0x00000008u);  // 32 skipped, 16 produced
  CHECK(S.a.top_on && S.a.feedback_seen[0] == 0x10u && S.a.feedback_seen[1] == 0x8u, "wrapped, paying");
  S.verdict(0xffffffffu, 0xfffffffeu);
  S.verdict(0x00000001u, 0x0000001cu);  // 2 skipped, 30 produced
  CHECK(!S.a.top_on && S.a.top_single_batches == 1, "wrapped, not paying");
  // modes 0 and 1 ignore the feedback
  for (int mode = 0; mode <= 1; mode++) {
    Sched M;
    M.create(W1, H1, NL1, 4, "2");
    M.a.top_mode = mode;
    M.verdict(1, 1000);
    CHECK(M.a.top_on && M.a.feedback_seen[0] == 0 && M.a.feedback_seen[1] == 0 && M.a.top_single_batches == 0, "mode %d read the feedback", mode);
    M.a.top_on = false;
    CHECK(M.wanted(2) == (mode == 1) && !M.wanted(0), "mode %d wanted", mode);
  }
}

// ---- a new frame size ------------------------------------------------------------------------------------------------------
void check_new_size() {
  Sched S;
  S.create(W1, H1, NL1, 4, "2:0,65:trace");
  S.trace = nullptr;
  level0(S, 74, {60, 900}, {74, 100});
  CHECK(run_window(S) && S.a.tile_h_pref[0] == 40 && S.a.cut_pref[0] == 61, "learned");
  S.step();
  S.verdict(3, 15);
  S.words[0] = 3;
  S.words[1] = 15;
  S.frame_size(640, 480);
  const OrbxAdapt& a = S.a;
  bool clean = a.learn_w == 640 && a.learn_h == 480 && a.need_batches == 0 && a.need_window == 2 && a.retiles == 0;
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
    clean = clean && !a.need_cur[l] && !a.need_prev[l] && !a.tile_h_pref[l] && !a.cut_pref[l];
    for (int b = 0; b < ORBX_FILL_BUCKETS; b++) clean = clean && !a.fill_cur[l][b] && !a.fill_prev[l][b] && !a.fill_last[l][b];
  }
  for (int i = 2; i < ORBX_FEEDBACK_WORDS; i++) clean = clean && S.words[i] == 0;
  CHECK(clean, "something learned survived");
  // the running totals, the verdict and the switches are not learned from a frame size
  CHECK(S.words[0] == 3 && S.words[1] == 15 && !a.top_on && a.feedback_seen[1] == 15 && a.cut_force[1] == 65 && a.split_trace, "more than the learned was cleared");
}

// ---- the fields behind ORBX_TOP_ROWS' number -------------------------------------------------------------------------------
void check_parser() {
  auto parsed = [](const char* s) {
    OrbxAdapt a;
    first_split_fields(a, s);
    return a;
  };
  auto forces = [](const OrbxAdapt& a) {
    int n = 0;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) n += a.cut_force[l] != 0;
    return n;
  };
  for (const char* s : {(const char*)nullptr, "", "2", "0"}) {
    const OrbxAdapt a = parsed(s);
    CHECK(a.first_split && !a.split_trace && a.early_band && forces(a) == 0, "defaults for %s", s ? s : "(unset)");
  }
  OrbxAdapt a = parsed("2:equal");
  CHECK(!a.first_split && !a.split_trace && a.early_band && forces(a) == 0, "2:equal");
  a = parsed("2:trace:late");
  CHECK(a.first_split && a.split_trace && !a.early_band && forces(a) == 0, "2:trace:late");
  a = parsed("2:68,65,0,61");
  CHECK(a.cut_force[0] == 68 && a.cut_force[1] == 65 && a.cut_force[2] == 0 && a.cut_force[3] == 61 && forces(a) == 3, "2:68,65,0,61");
  CHECK(a.first_split && !a.split_trace && a.early_band, "a list set a switch");
  a = parsed("2:70000");
  CHECK(a.cut_force[0] == 65535 && forces(a) == 1, "2:70000 -> %d", a.cut_force[0]);
  a = parsed("2:-5");
  CHECK(a.cut_force[0] == 0 && forces(a) == 0, "2:-5 -> %d", a.cut_force[0]);
  a = parsed("2:trace:68,65:equal");
  CHECK(a.split_trace && !a.first_split && a.cut_force[0] == 68 && a.cut_force[1] == 65 && forces(a) == 2, "fields in any order");
  // a list longer than ORBX_MAX_LEVELS: the first ORBX_MAX_LEVELS numbers, nothing written behind the array (the
  // sanitizer's business), and the fields after the list are still read
  struct {
    OrbxAdapt a;
    int behind = 12345;
  } box;
  first_split_fields(box.a, "2:1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20:late");
  bool in_order = true;
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) in_order = in_order && box.a.cut_force[l] == l + 1;
  CHECK(in_order && box.behind == 12345 && !box.a.early_band && box.a.cut_pref[0] == 0, "a long list");
}

// ---- the trace lines (tests and tools/adapt_probe.py parse them) -----------------------------------------------------------
void check_trace() {
  char* text = nullptr;
  size_t len = 0;
  FILE* f = open_memstream(&text, &len);
  Sched S;
  S.trace = f;
  S.create(W1, H1, 1, 4, "2:trace");
  CHECK(S.a.split_trace, "trace");
  level0(S, 74, {60, 900}, {74, 100});
  CHECK(run_window(S), "re-tile");
  std::fclose(f);
  const char* want =
      "orbx split: batch 1 level 0 need 74 depth 80 cut 0 -> 61 (14400 -> 10872 milli-groups) fill rows: 60:1800 76:200\n"
      "orbx split: batch 1 re-tile 1\n"
      "orbx early band: level 0 cut 61 first pass ended at 101, now ends at 84, band 17 rows: split\n";
  CHECK(text && !std::strcmp(text, want), "trace:\n%s", text ? text : "(none)");
  std::free(text);
}

// ---- seeded replay ---------------------------------------------------------------------------------------------------------
struct Rng {  // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};
uint64_t fold(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001B3ull; }  // FNV-1a over 64-bit words

// A stream of `batches` batches: every level's caps fill around a row that drifts and now and then jumps; frames are
// counted by fill row in the rows just above it; the verdict's totals advance with a skip share that changes by
// regime and wrap more than once; some batches report nothing, and now and then the frame size "changes".
void seeded(int w, int h, int nlevels, int impl, const char* fields, uint64_t seed, int batches, uint64_t* hash, int* retiles) {
  Sched S;
  S.create(w, h, nlevels, impl, fields);
  Rng r{seed};
  int base[ORBX_MAX_LEVELS], spread[ORBX_MAX_LEVELS];
  for (int l = 0; l < nlevels; l++) base[l] = 8 + (int)r.below((uint32_t)S.plan.L[l].h), spread[l] = 1 + (int)r.below(12);
  uint32_t skipped = 0, produced = 0, share = 50;
  uint64_t hsh = 0xcbf29ce484222325ull;
  int trues = 0;
  for (int k = 0; k < batches; k++) {
    if (r.below(97) == 0)  // a jump: another scene
      for (int l = 0; l < nlevels; l++) base[l] = 4 + (int)r.below((uint32_t)S.plan.L[l].h + 20), spread[l] = 1 + (int)r.below(16);
    if (r.below(7) == 0) {  // a drift of one level
      const int l = (int)r.below((uint32_t)nlevels);
      base[l] = std::max(1, base[l] + (int)r.below(9) - 4);
    }
    if (r.below(211) == 0) share = r.below(101);
    if (r.below(1500) == 0) skipped += 0x7fff0000u, produced += 0x60000000u;
    if (r.below(4001) == 0) S.frame_size(w, h), S.rebuild();
    clear_words(S);
    if (r.below(16) != 0)
      for (int l = 0; l < nlevels; l++) {
        if (r.below(23) == 0) continue;  // this level reports nothing
        const int frames = 1 + (int)r.below(64);
        uint32_t need = 0;
        for (int f = 0; f < frames; f++) {
          const int row = std::max(1, base[l] - (int)r.below((uint32_t)spread[l]));
          need = std::max<uint32_t>(need, (uint32_t)row);
          S.words[ORBX_FEEDBACK_HIST + l * ORBX_FILL_BUCKETS + fill_bucket(std::min(row, S.plan.L[l].h))]++;
        }
        S.words[2 + l] = need;
      }
    const bool retile = S.step();
    if (S.wanted(2)) {  // a two-pass batch reports its levels
      const uint32_t levels = 1 + r.below(64 * (uint32_t)nlevels), sk = (uint32_t)((uint64_t)levels * share / 100);
      skipped += sk, produced += levels - sk;
    }
    if (r.below(5) != 0) S.verdict(skipped, produced);  // (else the words have not arrived yet)
    trues += retile;
    hsh = fold(hsh, retile);
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) hsh = fold(fold(fold(hsh, (uint64_t)S.a.tile_h_pref[l]), (uint64_t)S.a.cut_pref[l]), (uint64_t)S.a.early_rows[l]);
    hsh = fold(fold(fold(hsh, S.a.top_on), (uint64_t)S.a.need_window), (uint64_t)S.a.retiles);
  }
  *hash = hsh;
  *retiles = trues;
}

void check_seeded() {
  // expected: recorded from the scheduler as it stood inside orbx_api.cpp, before it moved to orbx_adapt.h
  const struct {
    const char* name;
    int w, h, nlevels, impl;
    const char* fields;
    uint64_t seed, hash;
    int retiles;
  } runs[] = {
      {"1241x376 streaming", W1, H1, NL1, 4, "2", 0x9E3779B97F4A7C15ull, 0x25653ff0453dfb4cull, 420},
      {"1241x376 tile", W1, H1, NL1, 3, "2", 0xD1B54A32D192ED03ull, 0xbf2f416c4b6e07e2ull, 250},
      {"160x160 streaming", W2, H2, NL2, 4, "2:0,0,30", 0x8CB92BA72F3D8DD7ull, 0xbc138051dccec337ull, 364},
  };
  for (const auto& run : runs) {
    uint64_t hash = 0;
    int retiles = 0;
    seeded(run.w, run.h, run.nlevels, run.impl, run.fields, run.seed, 20000, &hash, &retiles);
    std::printf("seeded %s: hash 0x%016" PRIx64 ", %d re-tiles\n", run.name, hash, retiles);
    CHECK(hash == run.hash && retiles == run.retiles, "seeded %s: expected 0x%016" PRIx64 ", %d re-tiles", run.name, run.hash, run.retiles);
  }
}

}  // namespace

int main() {
  check_windows();
  check_heights();
  check_group_rounding();
  check_cut();
  check_forced();
  check_early_bands();
  check_short_levels();
  check_verdict();
  check_new_size();
  check_parser();
  check_trace();
  check_seeded();
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
