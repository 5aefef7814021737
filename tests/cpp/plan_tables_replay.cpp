// plan_tables_replay.cpp -- host-only replay of everything the main path's kernels read of a frame size
// (csrc/orbx_tables.h: plan_with_taps, build_tile_tables): the resize taps and the levels' win8, the blur tile map, the
// FAST band map, the seven tile tables, the levels the second pass may skip and the rows the first pass ends at.  Every
// (frame size, scale factor, switches, scheduler state) case is folded, table byte by table byte, into one hash per
// frame size whose expected value was recorded from set_plan as it stood BEFORE the sequence moved into the header
// (inside orbx_api.cpp, interleaved with the uploads), so the move itself is pinned.  Scripted cases assert what no
// batch on a device can reach: learned tile rows that overflow the FAST pool are forgotten, and every table that
// overflows its pool is refused with its message.  Calls the code the library itself runs.  Test infrastructure only;
// built with -fsanitize=address,undefined by tests/test_cpp_plan_tables.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// ---- the sequence under test ------------------------------------------------------------------------------------------
#include "../../visual-odometry-gpu_amd/csrc/orbx_tables.h"
// ---- end of the sequence under test -----------------------------------------------------------------------------------

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

uint64_t fold(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001B3ull; }  // FNV-1a over 64-bit words
const uint64_t kSeed = 0xcbf29ce484222325ull;

template <class T>
uint64_t fold_ints(uint64_t h, const T* v, size_t n) {
  for (size_t i = 0; i < n; i++) h = fold(h, (uint64_t)(int64_t)v[i]);
  return h;
}
// the bytes of n records of 8 k bytes each (no padding in either table's record)
template <class T>
uint64_t fold_bytes(uint64_t h, const T* v, size_t n) {
  static_assert(sizeof(T) % 8 == 0, "whole 64-bit words");
  for (size_t i = 0; i < n; i++) {
    uint64_t words[sizeof(T) / 8];
    std::memcpy(words, &v[i], sizeof(T));
    for (uint64_t word : words) h = fold(h, word);
  }
  return h;
}
static_assert(sizeof(OrbxResizeTap) == 8 && sizeof(OrbxTileDesc) == 64, "records without padding");

uint64_t fold_plan_and_taps(uint64_t h, const OrbxPlan& P, const std::vector<OrbxResizeTap>& taps) {
  h = fold(h, (uint64_t)P.nlevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) h = fold(h, (uint64_t)(int64_t)P.L[l].win8);
  h = fold(h, taps.size());
  return fold_bytes(h, taps.data(), taps.size());
}

// (make_tilemap writes the strips per row of the plan's levels only: what a larger plan left behind them is never read)
uint64_t fold_tables(uint64_t h, const OrbxPlanTables& T, int nlevels) {
  h = fold_ints(h, T.tm_blur.begin, ORBX_MAX_LEVELS + 1);
  h = fold_ints(h, T.tm_blur.tiles_x, nlevels);
  const OrbxBandMap& bm = T.bm_fast;
  h = fold(h, (uint64_t)(int64_t)bm.nbands);
  h = fold_ints(h, bm.band_begin, ORBX_MAX_BANDS + 1);
  h = fold_ints(h, bm.tiles_x, ORBX_MAX_LEVELS);
  h = fold_ints(h, bm.tiles_y, ORBX_MAX_LEVELS);
  h = fold_ints(h, bm.tile_h, ORBX_MAX_LEVELS);
  h = fold_ints(h, bm.xprefix, ORBX_MAX_LEVELS + 1);
  h = fold_ints(h, &bm.first_h[0][0], 2 * ORBX_MAX_LEVELS);
  for (int i = 0; i < kTileTables; i++) {
    h = fold(h, T.tiles[i].size());
    h = fold_bytes(h, T.tiles[i].data(), T.tiles[i].size());
  }
  h = fold(h, (uint64_t)(int64_t)T.top_levels.n);
  h = fold_ints(h, T.top_levels.stat_index, ORBX_MAX_LEVELS);
  h = fold_ints(h, T.top_levels.rows, ORBX_MAX_LEVELS);
  return fold_ints(h, T.top_levels.cap, ORBX_MAX_LEVELS);
}

// what a failing or a succeeding call leaves in the record
uint64_t fold_record(uint64_t h, const OrbxAdapt& a) {
  h = fold_ints(h, a.early_rows, ORBX_MAX_LEVELS);
  h = fold_ints(h, a.tile_h_pref, ORBX_MAX_LEVELS);
  h = fold_ints(h, a.cut_pref, ORBX_MAX_LEVELS);
  return fold(h, a.prefs_applied);
}

bool same_tables(const OrbxPlanTables& A, const OrbxPlanTables& B, int nlevels) {
  return fold_tables(kSeed, A, nlevels) == fold_tables(kSeed, B, nlevels);
}

orbx_params params_for(float scale, int nlevels, int w, int h) {
  orbx_params p{};
  p.nfeatures = 1000;
  p.scale_factor = scale;
  p.nlevels = nlevels;
  p.threshold = 20;
  p.n = 9;
  p.nms_window = 3;
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

// a frame size as a context created for exactly that size sees it: the plan with its taps, the pools' capacities
struct Frame {
  orbx_params p{};
  OrbxPlan plan{};
  std::vector<OrbxResizeTap> taps;
  OrbxTableCapacity cap{};
};
// the most levels, up to `nlevels`, that the library accepts for the size
bool make_frame(int w, int h, float scale, int nlevels, int fast_impl, int blur_impl, Frame* F) {
  std::string why;
  for (; nlevels >= 1; nlevels--) {
    F->p = params_for(scale, nlevels, w, h);
    OrbxPlan M;
    if (build_plan(F->p, w, h, &M, &why, fast_impl) != ORBX_OK) continue;
    if (table_capacity(F->p, M, fast_impl, blur_impl, &F->cap, &why) != ORBX_OK) continue;
    return plan_with_taps(F->p, w, h, fast_impl, &F->plan, &F->taps, &why) == ORBX_OK;
  }
  return false;
}

// ---- the scheduler states that change a table ----------------------------------------------------------------------------
void hist_add(uint32_t* hist, int fill_row, uint32_t n) { hist[fill_bucket(fill_row)] += n; }
void learned_rows(OrbxAdapt& a) {
  const int rows[] = {33, 28, 40, 20, 16, 0, 24, 17};
  for (int l = 0; l < 8; l++) a.tile_h_pref[l] = rows[l];
}
void chosen_cut(OrbxAdapt& a) {  // tile rows of 40: a first pass of 80 rows, cut at 61 (level 0) and at 54 (level 1)
  a.tile_h_pref[0] = a.tile_h_pref[1] = 40;
  a.cut_pref[0] = 61;
  a.cut_pref[1] = 54;
}
struct State {
  const char* name;
  bool pipeline;  // the top-rows-first pipeline can run (with a first pass of at least one tile row)
  void (*set)(OrbxAdapt& a);
};
const State kStates[] = {
    {"fresh", true, [](OrbxAdapt&) {}},
    {"learned tile rows", true, [](OrbxAdapt& a) { learned_rows(a); }},
    {"learned tile rows, pipeline off", false, [](OrbxAdapt& a) { learned_rows(a); }},
    {"chosen cut", true, [](OrbxAdapt& a) { chosen_cut(a); }},
    {"forced cut", true, [](OrbxAdapt& a) { first_split_fields(a, "2:68,65,0,61"); }},
    {"forced cut over learned rows", true, [](OrbxAdapt& a) { learned_rows(a), first_split_fields(a, "2:30,0,55,12,9"); }},
    {"2:equal", true, [](OrbxAdapt& a) { chosen_cut(a), first_split_fields(a, "2:equal"); }},
    {"2:late, forced", true, [](OrbxAdapt& a) { first_split_fields(a, "2:late:68,87,86"); }},
    // 900 of 1000 frames fill by row 60, within tile row 0: the band of level 0 pays; on level 1 nobody does
    {"histograms: band pays", true, [](OrbxAdapt& a) {
       chosen_cut(a);
       hist_add(a.fill_last[0], 60, 900), hist_add(a.fill_last[0], 74, 100);
       hist_add(a.fill_last[1], 70, 1000);
     }},
    {"2:late over the same", true, [](OrbxAdapt& a) {
       chosen_cut(a), first_split_fields(a, "2:late");
       hist_add(a.fill_last[0], 60, 900), hist_add(a.fill_last[0], 74, 100);
     }},
    // every frame fills below the cut: every frame would pay the warm-up rows of one more band
    {"histograms: band does not pay", true, [](OrbxAdapt& a) {
       chosen_cut(a);
       hist_add(a.fill_last[0], 75, 1000), hist_add(a.fill_last[1], 75, 1000);
     }},
};

struct Counts {
  long long cases = 0, moved_cut = 0, split_band = 0, kept_band = 0, shorter_rows = 0;
  long long win8[4] = {};  // levels above 0 by their resize mode
};

// ---- every case of one frame size ------------------------------------------------------------------------------------------
uint64_t replay_size(int w, int h, int nlevels, Counts* n) {
  uint64_t hash = kSeed;
  OrbxPlanTables T;  // (reused from case to case, as the library's is from re-tile to re-tile)
  for (float scale : {1.2f, 1.5f, 2.0f})
    for (int fast_impl : {4, 3})
      for (int blur_impl : {1, 2, 3}) {
        Frame F;
        const bool ok = make_frame(w, h, scale, nlevels, fast_impl, blur_impl, &F);
        CHECK(ok, "%d x %d at scale %.1f: no plan", w, h, (double)scale);
        if (!ok) continue;
        const uint64_t plan_hash = fold_plan_and_taps(kSeed, F.plan, F.taps);
        if (fast_impl == 4 && blur_impl == 1)
          for (int l = 1; l < F.plan.nlevels; l++) n->win8[F.plan.L[l].win8 & 3]++;
        const int R = F.p.nms_window / 2;
        OrbxBandMap dflt;
        std::string why;
        CHECK(make_bandmap(F.plan, R, &dflt, &why, fast_impl == 4, nullptr) == ORBX_OK, "default rows: %s", why.c_str());
        for (int grouped = 0; grouped <= 1; grouped++)
          for (int top = 0; top <= 3; top++)
            for (const State& s : kStates) {
              OrbxAdapt a;
              s.set(a);
              const OrbxTableSwitches sw{fast_impl, blur_impl, top, grouped != 0, s.pipeline && top > 0};
              const int st = build_tile_tables(F.plan, R, sw, F.cap, a, nullptr, &T, &why);
              CHECK(st == ORBX_OK, "%d x %d scale %.1f kernels %d/%d top %d %s: %s", w, h, (double)scale, fast_impl,
                    blur_impl, top, s.name, why.c_str());
              hash = fold(hash, plan_hash);
              hash = fold(hash, (uint64_t)st);
              if (st != ORBX_OK) continue;
              hash = fold_record(fold_tables(hash, T, F.plan.nlevels), a);
              n->cases++;
              bool cut = false, split = false, kept = false, shorter = false;
              for (int l = 0; l < F.plan.nlevels; l++) {
                const int late = pyrblur_first_pass_rows(F.plan, T.bm_fast, l, top);
                cut |= T.bm_fast.first_h[l][0] > 0;
                split |= a.early_rows[l] < late;
                kept |= a.early_rows[l] == late && pyrblur_early_rows(F.plan, T.bm_fast, l, top, R) < late;
                shorter |= T.bm_fast.tile_h[l] < dflt.tile_h[l];
              }
              n->moved_cut += cut, n->split_band += split, n->kept_band += kept, n->shorter_rows += shorter;
            }
      }
  return hash;
}

// the smallest square the library accepts for the default parameters (scanned from 8 x 8)
int smallest_size(int nlevels) {
  for (int s = 8; s <= 4096; s++) {
    OrbxPlan P;
    OrbxBandMap bm;
    std::string why;
    const orbx_params p = params_for(1.2f, nlevels, s, s);
    if (build_plan(p, s, s, &P, &why, 4) == ORBX_OK && make_bandmap(P, p.nms_window / 2, &bm, &why, true, nullptr) == ORBX_OK)
      return s;
  }
  return 0;
}

// ---- what no batch can reach: pools that are too small --------------------------------------------------------------------
const char* const kMessage[kTileTables] = {
    "FAST tile table exceeds pool",  "blur tile table exceeds pool", "pyramid tile table exceeds pool", "strip table exceeds pool",
    "strip table exceeds pool",      "strip table exceeds pool",     "strip table exceeds pool"};
static_assert(T_FAST == 0 && T_BLUR == 1 && T_PYR2 == 2 && T_PYRBLUR == 3 && T_PYRBLUR_SMALL == 4 && T_PYRBLUR_TOP == 5 &&
                  T_PYRBLUR_REST == 6 && kTileTables == 7, "the messages above are in the tables' order");
size_t& pool_of(OrbxTableCapacity& cap, int table) { return table == T_FAST ? cap.fast : table == T_PYRBLUR_SMALL ? cap.small : cap.frame; }

uint64_t scripted(int w, int h, int nlevels, int fast_impl, uint64_t hash, int* refused_by) {
  Frame F;
  // (k_blur4's strip table, the smallest of the tables that share a pool's size: it is built first, and a larger one
  // would be the table refused wherever a first-pass or second-pass strip table is one entry over)
  const bool ok = make_frame(w, h, 1.2f, nlevels, fast_impl, 3, &F);
  CHECK(ok, "%d x %d: no plan", w, h);
  if (!ok) return hash;
  const int R = F.p.nms_window / 2;
  const OrbxTableSwitches sw{fast_impl, 3, 2, true, true};
  std::string why;
  // the tables of a fresh record, and of the learned rows where the pool holds them
  OrbxAdapt fresh, learned;
  learned_rows(learned);
  OrbxPlanTables Tf, Tl, T;
  CHECK(build_tile_tables(F.plan, R, sw, F.cap, fresh, nullptr, &Tf, &why) == ORBX_OK, "fresh: %s", why.c_str());
  CHECK(build_tile_tables(F.plan, R, sw, F.cap, learned, nullptr, &Tl, &why) == ORBX_OK, "learned: %s", why.c_str());
  const size_t need = Tl.tiles[T_FAST].size(), dflt = Tf.tiles[T_FAST].size();
  CHECK(need > dflt && learned.prefs_applied && learned.tile_h_pref[0] == 33, "%d x %d: the learned rows need %zu units, the default %zu", w, h, need, dflt);
  // a FAST pool one entry short of the learned rows: they are forgotten, and the tables are the fresh record's
  OrbxTableCapacity cap = F.cap;
  cap.fast = need - 1;
  OrbxAdapt a;
  learned_rows(a);
  a.cut_pref[0] = 47;  // (of the 66 rows of the learned first pass; a cut goes with the rows: it needs prefs_applied)
  const int st = build_tile_tables(F.plan, R, sw, cap, a, nullptr, &T, &why);
  CHECK(st == ORBX_OK, "%d x %d: learned rows over the pool: %s", w, h, why.c_str());
  bool forgotten = !a.prefs_applied;
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) forgotten = forgotten && a.tile_h_pref[l] == 0 && a.early_rows[l] == fresh.early_rows[l];
  CHECK(forgotten, "%d x %d: the learned rows were kept", w, h);
  CHECK(same_tables(T, Tf, F.plan.nlevels) && T.tiles[T_FAST].size() == dflt, "%d x %d: not the tables of a fresh record", w, h);
  hash = fold_record(fold_tables(fold(hash, (uint64_t)st), T, F.plan.nlevels), a);
  // ... and one short of the default rows too: refused
  cap.fast = dflt - 1;
  OrbxAdapt b;
  learned_rows(b);
  CHECK(build_tile_tables(F.plan, R, sw, cap, b, nullptr, &T, &why) == ORBX_ERR_UNSUPPORTED && why == kMessage[T_FAST], "FAST pool one short: %s", why.c_str());
  hash = fold_record(hash, b);
  // every table with a pool one entry short of its count: refused with the message of the first table, in the
  // order they are built in, that does not fit (tables share the pools' sizes)
  const int order[kTileTables] = {T_BLUR, T_PYRBLUR, T_PYRBLUR_TOP, T_PYRBLUR_REST, T_PYRBLUR_SMALL, T_PYR2, T_FAST};
  for (int table = 0; table < kTileTables; table++) {
    const size_t count = Tf.tiles[table].size();
    CHECK(count > 0, "table %d is empty", table);
    if (count == 0) continue;
    OrbxTableCapacity c1 = F.cap;
    pool_of(c1, table) = count - 1;
    int first = -1;
    for (int t : order)
      if (first < 0 && Tf.tiles[t].size() > pool_of(c1, t)) first = t;
    OrbxAdapt x;
    why.clear();
    const int s1 = build_tile_tables(F.plan, R, sw, c1, x, nullptr, &T, &why);
    CHECK(s1 == ORBX_ERR_UNSUPPORTED && first >= 0 && why == kMessage[first], "table %d with a pool of %zu for %zu entries: status %d, %s", table, count - 1, count, s1, why.c_str());
    CHECK(why == kMessage[table], "table %d refused with another table's message: %s", table, why.c_str());
    if (first == table) refused_by[table]++;
    hash = fold_record(fold(fold(hash, (uint64_t)s1), (uint64_t)first), x);
  }
  return hash;
}

}  // namespace

int main() {
  // expected: recorded from set_plan as it stood inside orbx_api.cpp, before the sequence moved to orbx_tables.h
  const int small = smallest_size(8);
  std::printf("smallest size: %d x %d\n", small, small);
  CHECK(small == 27, "the smallest size the library accepts moved");
  const struct {
    const char* name;
    int w, h, nlevels;
    uint64_t hash;
  } sizes[] = {
      {"1241x376", 1241, 376, 8, 0x7a9d0cae9b7cf44dull},
      {"1920x1080", 1920, 1080, 8, 0x1ec336d73ebef1d5ull},
      {"160x160", 160, 160, 12, 0xb0d8f77b6ebebcbdull},  // one tile row on the upper levels
      {"645x487", 645, 487, 8, 0xdc485b1b215e85fdull},   // odd, and the width no multiple of 4
      {"smallest", small, small, 8, 0x277f0d8d78cabaa5ull},
  };
  Counts n;
  for (const auto& s : sizes) {
    const uint64_t hash = replay_size(s.w, s.h, s.nlevels, &n);
    std::printf("replay %s: hash 0x%016" PRIx64 "\n", s.name, hash);
    CHECK(hash == s.hash, "replay %s: expected 0x%016" PRIx64, s.name, s.hash);
  }
  std::printf("%lld cases: %lld moved a cut, %lld split an early band, %lld kept one, %lld with shorter tile rows; levels by win8: %lld / %lld / %lld\n",
              n.cases, n.moved_cut, n.split_band, n.kept_band, n.shorter_rows, n.win8[0], n.win8[1], n.win8[3]);
  CHECK(n.moved_cut > 0 && n.split_band > 0 && n.kept_band > 0 && n.shorter_rows > 0, "a state changed no table");
  CHECK(n.win8[0] > 0 && n.win8[1] > 0 && n.win8[3] > 0 && n.win8[2] == 0, "a resize mode no level took");
  int refused_by[kTileTables] = {};
  uint64_t hash = kSeed;
  hash = scripted(1241, 376, 8, 4, hash, refused_by);
  hash = scripted(1241, 376, 8, 3, hash, refused_by);
  hash = scripted(645, 487, 8, 4, hash, refused_by);
  std::printf("scripted: hash 0x%016" PRIx64 "\n", hash);
  CHECK(hash == 0xfe11737ed650c628ull, "scripted: the record or the tables after a refusal changed");
  for (int t = 0; t < kTileTables; t++)
    // (the strip tables of the two passes have no more strips than the whole table, which is built before them, shares
    // their pool's size and has their message)
    if (t != T_PYRBLUR_TOP && t != T_PYRBLUR_REST)
      CHECK(refused_by[t] > 0, "table %d was never the one refused", t);
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
