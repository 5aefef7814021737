// orbx_tables.h -- everything the main path's kernels read of a frame size, built in ONE place: the plan with its
// resize taps (plan_with_taps) and, from it, the blur tile map, the FAST band map, the seven tile tables and the levels
// the second pass may skip (build_tile_tables).  Host arithmetic on plain data: no HIP, no getenv.  orbx_api.cpp's
// set_plan reads the switches, calls the two and copies what they made to the device; the CPU tests call the very
// same two (tests/cpp/plan_tables_replay.cpp pins the bytes of every table, adapt_replay.cpp and
// plan_capacity_sweep.cpp build their tables through them).
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "orbx_adapt.h"

// the per-workgroup tile descriptor tables (see OrbxTileDesc) of a plan
enum {
  T_FAST,  // one frame, band-major
  T_BLUR,
  T_PYR2,
  T_PYRBLUR,  // fused pyramid + blur strips
  // the same strips cut into short row bands: few frames per call (the reference's one-frame call shape)
  // fill the chip only with many short waves, where a large batch wants few tall ones
  T_PYRBLUR_SMALL,
  // top-rows-first pipeline: the strips of the first pass and of the second one
  T_PYRBLUR_TOP,
  T_PYRBLUR_REST,
  kTileTables
};

// the switches the sequence reads (orbx_api.cpp fills them from the environment and the context)
struct OrbxTableSwitches {
  int fast_impl, blur_impl;  // ORBX_FAST_IMPL, ORBX_BLUR_IMPL
  int top_rows;              // ORBX_TOP_ROWS' number
  bool grouped;              // ORBX_PYR_GROUP > 0: the fused kernel's strips heaviest first
  bool prefs_apply;          // the top-rows-first pipeline can run at all (tile_prefs_apply)
};

struct OrbxPlanTables {
  OrbxTileMap tm_blur{};  // 5x5 /273 variant (LDS tile kernel)
  OrbxBandMap bm_fast{};
  std::vector<OrbxTileDesc> tiles[kTileTables];
  OrbxTopLevels top_levels{};  // the levels the second pass may skip
};

namespace orbx_tables {

using namespace orbx_adapt;

// entries of the pool of a table (OrbxTableCapacity, orbx_plan.h)
inline size_t tile_table_capacity(const OrbxTableCapacity& cap, int table) {
  return table == T_FAST ? cap.fast : table == T_PYRBLUR_SMALL ? cap.small : cap.frame;
}

// the plan of a frame size as the kernels read it: with the taps' verdict on every level's resize mode (win8)
inline int plan_with_taps(const orbx_params& p, int w, int h, int fast_impl, OrbxPlan* plan,
                          std::vector<OrbxResizeTap>* taps, std::string* why) {
  const int st = build_plan(p, w, h, plan, why, fast_impl);
  if (st != ORBX_OK) return st;
  make_taps(*plan, taps);
  return ORBX_OK;
}

// The tables of `plan` (plan_with_taps), each checked against its pool.  a: the scheduler's record -- what it has
// learned chooses the tile rows, the cut and the early bands, and this writes prefs_applied and early_rows (and
// forgets the learned tile rows that do not fit).  trace: where the early bands' decisions go, or NULL.  A failure
// leaves *out half built: the caller must not use it.
inline int build_tile_tables(const OrbxPlan& plan, int nms_radius, const OrbxTableSwitches& sw,
                             const OrbxTableCapacity& cap, OrbxAdapt& a, FILE* trace, OrbxPlanTables* out,
                             std::string* why) {
  OrbxBandMap& bm = out->bm_fast;
  const OrbxAdaptGeom geom{plan, bm, nms_radius, sw.fast_impl, sw.top_rows};
  auto too_large = [&](int table, const char* msg) {
    if (out->tiles[table].size() <= tile_table_capacity(cap, table)) return false;
    *why = msg;
    return true;
  };
  make_tilemap(plan, ORBX_BLUR_TW, ORBX_BLUR_TH, true, &out->tm_blur);
  // (the adaptive first pass's shorter tile rows only where the top-rows-first pipeline can run at all: with the
  // early exit or the fused kernel switched off every tile works, and the default rows have the smaller halo share)
  a.prefs_applied = sw.prefs_apply;
  int st = make_bandmap(plan, nms_radius, &bm, why, sw.fast_impl == 4, a.prefs_applied ? a.tile_h_pref : nullptr);
  if (a.prefs_applied && (st != ORBX_OK || (size_t)bm.band_begin[bm.nbands] > cap.fast)) {
    // The learned tile rows give a table the pool cannot hold (the FAST table's capacity is an upper bound over every
    // preference, orbx_plan.h: this is a second line of defence).  What was learned is only a partition of the work:
    // forget it, take the default rows and run the batch -- a failure here would repeat with every batch of this size.
    forget_tile_rows(a);
    st = make_bandmap(plan, nms_radius, &bm, why, sw.fast_impl == 4, nullptr);
  }
  if (st != ORBX_OK) return st;
  // the first pass cut unevenly (same number of tile rows, same pool): where the chooser or a forced cut says so
  // (the first call above accepted these tile rows: this one cannot fail, and an illegal pair is ignored)
  int first[ORBX_MAX_LEVELS][2] = {};
  if (first_pass_heights(a, geom, first))
    (void)make_bandmap(plan, nms_radius, &bm, why, sw.fast_impl == 4, a.prefs_applied ? a.tile_h_pref : nullptr, first);
  const bool grouped = sw.grouped;
  const int top = sw.top_rows;
  blur_tiles_for_impl(sw.blur_impl, plan, &out->tiles[T_BLUR]);
  if (too_large(T_BLUR, "blur tile table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &out->tiles[T_PYRBLUR], grouped);
  if (too_large(T_PYRBLUR, "strip table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  choose_early_bands(a, geom, trace);
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &out->tiles[T_PYRBLUR_TOP], grouped, 1, &bm, top, a.early_rows);
  if (too_large(T_PYRBLUR_TOP, "strip table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &out->tiles[T_PYRBLUR_REST], grouped, 2, &bm, top, a.early_rows);
  if (too_large(T_PYRBLUR_REST, "strip table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  out->top_levels = OrbxTopLevels{};
  for (int l = 0; l < plan.nlevels; l++)
    if (pyrblur_first_pass_rows(plan, bm, l, top) < plan.L[l].h) {
      const int i = out->top_levels.n++;
      out->top_levels.stat_index[i] = l * ORBX_MAX_BANDS;
      out->top_levels.rows[i] = std::min(top, bm.tiles_y[l]);
      out->top_levels.cap[i] = plan.L[l].cap;
    }
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH_SMALL, &out->tiles[T_PYRBLUR_SMALL]);
  if (too_large(T_PYRBLUR_SMALL, "strip table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  build_frame_tiles(plan, ORBX_PYR2_TW, ORBX_PYR2_TH, true, &out->tiles[T_PYR2]);
  if (too_large(T_PYR2, "pyramid tile table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  build_fast_tiles(plan, bm, 0, 1, &out->tiles[T_FAST]);
  if (too_large(T_FAST, "FAST tile table exceeds pool")) return ORBX_ERR_UNSUPPORTED;
  return ORBX_OK;
}

}  // namespace orbx_tables
