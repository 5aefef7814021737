// orbx_adapt.h -- the scheduler of the batched path's first pass: ONE record of what it has learned and of its
// switches (OrbxAdapt), and the steps that change it, as pure functions of plain data.  No HIP, no getenv, no access
// to the pinned feedback buffer: orbx_api.cpp reads the environment, takes ONE snapshot of the feedback words per
// batch (a stale or torn word only misleads the heuristic for one batch -- results never depend on it -- so a
// snapshot taken a little earlier than the word-by-word reads it replaces is within that contract), and rebuilds the
// tile tables when a step says so.  Nothing here can change a result: only how a batch's work is partitioned.
// tests/cpp/adapt_replay.cpp replays scripted and seeded streams through these steps on the CPU.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "orbx_plan.h"

struct OrbxAdapt {
  // Top-rows-first pipeline (enqueue_batch): 0 never, 1 whenever eligible, 2 adaptive -- the second pass
  // counts the (frame, level)s it skipped / had to produce (d_feedback, running totals, written to the pinned
  // h_feedback by the last kernel of every two-pass batch and read WITHOUT waiting at the start of later ones); while
  // fewer than a quarter are skipped the batches run in one pass, and every 128th one probes again.
  int top_mode = 2;
  bool top_on = true;          // the adaptive verdict
  int top_single_batches = 0;  // one-pass batches since the verdict turned negative
  uint32_t feedback_seen[2] = {0, 0};
  // adaptive first pass (adapt_tile_rows): rows each level needed to fill its cap -- maximum of the current and of
  // the previous observation window --, the tile-row heights chosen from them (0: the default), bookkeeping
  uint32_t need_cur[ORBX_MAX_LEVELS] = {}, need_prev[ORBX_MAX_LEVELS] = {};
  int tile_h_pref[ORBX_MAX_LEVELS] = {};
  int need_batches = 0, need_window = 2, retiles = 0, learn_w = 0, learn_h = 0;
  bool prefs_applied = false;  // the current tile tables were built with tile_h_pref
  // unevenly cut first pass (adapt_tile_rows, orbx_plan.h: choose_first_cut): the frames of the current and of the
  // previous observation window counted by the row their caps filled in, and the rows of tile row 0 chosen from them
  // (0: equal halves).  Read when the context is created, from the fields behind ORBX_TOP_ROWS' number
  // (first_split_fields): equal halves only (A/B timing), the rows of tile row 0 forced per level (tests), a trace.
  uint32_t fill_cur[ORBX_MAX_LEVELS][ORBX_FILL_BUCKETS] = {}, fill_prev[ORBX_MAX_LEVELS][ORBX_FILL_BUCKETS] = {};
  int cut_pref[ORBX_MAX_LEVELS] = {}, cut_force[ORBX_MAX_LEVELS] = {};
  bool first_split = true, split_trace = false;
  // early band of the fused pyramid + blur kernel's second pass (orbx_plan.h: pyrblur_early_rows, early_band_pays):
  // the histograms the last observation window ended with -- set_plan decides per level from them when it builds the
  // tables, so only when adapt_tile_rows has them rebuilt --, and the row each level's first pass ends at in the
  // current tables (the end of tile row 1 + ORBX_TOP_MARGIN where there is no band).  ORBX_TOP_ROWS=2:late: no bands.
  uint32_t fill_last[ORBX_MAX_LEVELS][ORBX_FILL_BUCKETS] = {};
  int early_rows[ORBX_MAX_LEVELS] = {};
  bool early_band = true;
};

// the geometry a step looks at: the plan and the FAST band map of the current frame size, and what chose them
struct OrbxAdaptGeom {
  const OrbxPlan& plan;
  const OrbxBandMap& bm;
  int nms_radius, fast_impl, top_rows;  // top_rows: ORBX_TOP_ROWS' number
};

namespace orbx_adapt {

using namespace orbx_geom;

// most rows of a unit of the FAST kernel
inline int fast_unit_rows_max(int fast_impl, int nms_radius) {
  return fast_impl == 4 ? ORBX_FAST_UNIT_ROWS_MAX : orbx_fast3_tile_h(nms_radius);
}

// The switches of the unevenly cut first pass: fields behind the number of ORBX_TOP_ROWS, separated by colons and
// read when a context is created (the number itself is read once per process) --
//   ORBX_TOP_ROWS=2:equal          the two tile rows of the first pass stay equal halves (A/B timing)
//   ORBX_TOP_ROWS=2:68,65,0,61     rows of tile row 0 per level, forced (tests; 0: leave the level to the chooser)
//   ORBX_TOP_ROWS=2:trace          every decision of the chooser goes to stderr
//   ORBX_TOP_ROWS=2:late           no early bands: the first pyramid pass ends below tile row 1 on every level (A/B timing)
// e: the variable's value, or NULL
inline void first_split_fields(OrbxAdapt& a, const char* e) {
  e = e ? std::strchr(e, ':') : nullptr;
  while (e && *e == ':') {
    e++;
    if (!std::strncmp(e, "equal", 5)) {
      a.first_split = false;
    } else if (!std::strncmp(e, "trace", 5)) {
      a.split_trace = true;
    } else if (!std::strncmp(e, "late", 4)) {
      a.early_band = false;
    } else {
      for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end == e) break;
        a.cut_force[l] = (int)std::min<long>(std::max<long>(v, 0), 0xffff);
        e = end;
        if (*e != ',') break;
        e++;
      }
    }
    e = std::strchr(e, ':');
  }
}

// what was learned belongs to one frame size (feedback: the ORBX_FEEDBACK_WORDS words the device reports into)
inline void new_frame_size(OrbxAdapt& a, int w, int h, uint32_t* feedback) {
  a.learn_w = w;
  a.learn_h = h;
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.need_cur[l] = a.need_prev[l] = 0, a.tile_h_pref[l] = a.cut_pref[l] = 0;
  std::memset(a.fill_cur, 0, sizeof(a.fill_cur));
  std::memset(a.fill_prev, 0, sizeof(a.fill_prev));
  std::memset(a.fill_last, 0, sizeof(a.fill_last));
  for (int i = 2; i < ORBX_FEEDBACK_WORDS; i++) feedback[i] = 0;
  a.need_batches = 0;
  a.need_window = 2;
  a.retiles = 0;
}

// Top-rows-first pipeline: wanted for the next batch?  (Eligibility -- fused kernel, early exit on, large
// batch -- is checked where the launches are made.)
inline bool top_rows_wanted(const OrbxAdapt& a, int top_rows) {
  if (top_rows <= 0 || a.top_mode == 0) return false;
  return a.top_mode == 1 || a.top_on;
}
// adaptive mode: look at the totals the second passes have reported so far (no waiting: whatever has arrived).
// both: the pinned pair, skipped | produced << 32, from ONE 64-bit load (the device writes it as one 8-byte store of
// two lanes' dwords at best: a torn or stale pair, or a low half that has wrapped, only misleads this heuristic for
// one batch -- results never depend on it)
inline void top_rows_update(OrbxAdapt& a, uint64_t both) {
  if (a.top_mode != 2) return;
  const uint32_t sk = (uint32_t)both, pr = (uint32_t)(both >> 32);
  const uint32_t dsk = sk - a.feedback_seen[0], dpr = pr - a.feedback_seen[1];
  if (dsk + dpr > 0) {
    a.feedback_seen[0] = sk;
    a.feedback_seen[1] = pr;
    const bool pays = 4ull * dsk >= (unsigned long long)(dsk + dpr);  // a quarter of the levels skipped
    if (!pays && a.top_on) a.top_single_batches = 0;
    a.top_on = pays;
  }
  if (!a.top_on && ++a.top_single_batches >= 128) {  // probe again
    a.top_on = true;
    a.top_single_batches = 0;
  }
}

// Adaptive first pass.  The top-rows-first pipeline produces and searches the first ORBX_TOP_ROWS FAST tile rows of
// every level before anything else; with the default tile rows (<= 47 rows, balanced) that is ~90 rows per level,
// while a level's cap is typically full after 40-75 rows on the benchmark stream -- and everything a first-pass tile
// row holds beyond that row is work nobody reads.  The selection kernel reports, per level, the row in which the
// cap filled (maximum over the frames of a batch; the whole level if it never did); from the maximum over the last
// two observation windows, plus a margin, this picks SHORTER tile rows for the level, so that the first pass ends
// just below that row.  Only the partition of the work changes, never a result; a stream whose caps fill lower
// gets taller tile rows back (at most the default), and a frame whose cap is not full after the first pass is
// finished by the second one as always.  Returns true if the tile tables must be rebuilt (the caller forces
// set_plan, which waits for the batches in flight: it happens a few times per stream, not per batch).
// words: this batch's snapshot of the feedback words; prefs_apply: the top-rows-first pipeline can run at all
// (tile_prefs_apply); trace: where the chooser's decisions go, or NULL.
inline bool adapt_tile_rows(OrbxAdapt& a, const OrbxAdaptGeom& g, const uint32_t* words, bool prefs_apply,
                            long long batch_serial, FILE* trace) {
  if (!prefs_apply) return false;
  const int top = g.top_rows, nl = g.plan.nlevels;
  bool any = false;
  for (int l = 0; l < nl; l++) {
    const uint32_t v = words[2 + l];  // (whatever has arrived; a stale or torn word only misleads the heuristic)
    if (v) {
      a.need_cur[l] = std::max(a.need_cur[l], std::min<uint32_t>(v, (uint32_t)g.plan.L[l].h));
      any = true;
      // (the same batch may be counted twice, or not at all: only the shares matter)
      for (int b = 0; b < ORBX_FILL_BUCKETS; b++) {
        const uint32_t cnt = words[ORBX_FEEDBACK_HIST + l * ORBX_FILL_BUCKETS + b];
        a.fill_cur[l][b] += std::min<uint32_t>(cnt, 1u << 20);
      }
    }
  }
  if (!any || ++a.need_batches < a.need_window) return false;
  // end of an observation window (2, 4, 8, 16, then every 32 batches)
  a.need_batches = 0;
  a.need_window = std::min(2 * a.need_window, 32);
  bool change = false, grow = false;
  int want[ORBX_MAX_LEVELS] = {};
  for (int l = 0; l < nl; l++) {
    const uint32_t need = std::max(a.need_cur[l], a.need_prev[l]);
    a.need_prev[l] = a.need_cur[l];
    a.need_cur[l] = 0;
    if (need == 0) {
      want[l] = a.tile_h_pref[l];
      continue;
    }
    const int rows = (int)need + std::max(4, (int)need / 10);  // margin: the next frames' caps may fill a little lower
    // the default tile rows of the level (make_bandmap: <= dflt rows, balanced)
    const int dflt = orbx_fast3_tile_h(g.nms_radius), lh = g.plan.L[l].h;
    const int bal = (lh + (lh + dflt - 1) / dflt - 1) / ((lh + dflt - 1) / dflt);
    int hh = (rows + top - 1) / top;
    // the streaming FAST kernel walks whole groups of 7 centre rows (tile rows + 2 x NMS radius): a height that is
    // one or two rows into a new group gives them back where at least 3 rows of margin remain (measured: level 0 at
    // 40 instead of 41 rows, FAST -4.6 %, pyramid -2.9 %; rounding every level to a group boundary costs more than
    // it saves)
    if (g.fast_impl == 4) {
      const int over = (hh + 2 * g.nms_radius) % 7;
      if ((over == 1 || over == 2) && top * (hh - over) >= (int)need + 3) hh -= over;
    }
    if (hh >= bal || lh <= top * hh) hh = 0;  // the default rows do
    const int eff = hh ? hh : bal, cur = g.bm.tile_h[l], asked = a.tile_h_pref[l] ? a.tile_h_pref[l] : bal;
    // (a level that neither must grow nor gains three rows keeps its height when another level makes the tables change)
    want[l] = ((eff > cur && (int)need > top * cur) || eff + 2 < std::min(cur, asked)) ? hh : a.tile_h_pref[l];
    // the first pass has become too short for this stream -- caps fill BELOW it (the margin is used up): follow
    if (eff > cur && (int)need > top * cur) grow = true;
    // shrink only for a gain of three rows or more (`cur` may be taller than what was asked for: a level never has
    // more tile rows than the level above)
    else if (eff + 2 < std::min(cur, asked)) change = true;
  }
  // Where to cut the first pass.  Its two tile rows are equal halves by default, and a unit of tile row 1 may leave
  // only when the rows strictly above it hold the cap: no frame fills its cap in the upper half, so every frame
  // walks both.  With tile row 0 ending where most frames HAVE filled, the short tile row 1 runs for the others
  // alone (its units are dispatched a whole tile row of every frame later: the statistics are complete by then).
  // The cut per level comes from the fill-row histograms of the last two windows and the cost model of
  // choose_first_cut (orbx_plan.h), for the depth the level has after this decision; the tables are rebuilt for a
  // cut only if it saves a group or more per strip on some level, or if a cut in force has stopped paying.  Streaming
  // kernel only (the model counts its groups of 7 rows), and only where the fused selection reports the histograms.
  const bool heights_change = grow || change;
  const bool split = a.first_split && top == 2 && g.fast_impl == 4;
  const int R = g.nms_radius;
  int cut_want[ORBX_MAX_LEVELS] = {};
  bool cut_change = false;
  for (int l = 0; l < nl; l++) {
    uint32_t hist[ORBX_FILL_BUCKETS];
    uint64_t total = 0;
    for (int b = 0; b < ORBX_FILL_BUCKETS; b++) {
      hist[b] = a.fill_cur[l][b] + a.fill_prev[l][b];
      a.fill_last[l][b] = hist[b];  // (what set_plan decides the early bands from, if this window has it called)
      a.fill_prev[l][b] = a.fill_cur[l][b];
      a.fill_cur[l][b] = 0;
      total += hist[b];
    }
    if (!split || a.cut_force[l] > 0 || g.bm.tiles_y[l] < 2) continue;
    const int dflt = orbx_fast3_tile_h(R), lh = g.plan.L[l].h;
    const int bal = (lh + (lh + dflt - 1) / dflt - 1) / ((lh + dflt - 1) / dflt);
    const int th_after = heights_change ? (want[l] ? want[l] : bal) : g.bm.tile_h[l];
    const int depth = 2 * th_after;
    // (new tile-row heights void the cut in force: its pair no longer adds up to the depth)
    const int in_force = !heights_change && g.bm.first_h[l][0] > 0 ? g.bm.first_h[l][0] : 0;
    int cost_new = 0;
    const int cut_new = total && lh > depth ? choose_first_cut(hist, depth, R, ORBX_FAST_UNIT_ROWS_MAX, &cost_new) : 0;
    const int cost_now = first_pass_cost_milli(hist, depth, in_force ? in_force : depth / 2, R);
    if (!total || lh <= depth) cost_new = cost_now;
    const bool pays = cost_now - cost_new >= 1000, stopped = in_force && !cut_new && cost_now > cost_new;
    cut_want[l] = heights_change || pays || stopped ? cut_new : a.cut_pref[l];
    if (cut_want[l] != in_force && (pays || stopped)) cut_change = true;
    if (trace) {
      fprintf(trace, "orbx split: batch %lld level %d need %u depth %d cut %d -> %d (%d -> %d milli-groups) fill rows:",
              batch_serial, l, a.need_prev[l], depth, in_force, cut_want[l], cost_now, cost_new);
      for (int b = 0; b < ORBX_FILL_BUCKETS; b++)
        if (hist[b]) fprintf(trace, " %d:%u", ORBX_FILL_BUCKET_ROWS * (b + 1), hist[b]);
      fprintf(trace, "\n");
    }
  }
  if (!grow && !change && !cut_change) return false;
  if (!grow && a.retiles >= 4 && a.need_window < 32) return false;  // (settle first)
  for (int l = 0; l < nl; l++) a.tile_h_pref[l] = want[l], a.cut_pref[l] = cut_want[l];
  a.retiles++;
  if (trace) fprintf(trace, "orbx split: batch %lld re-tile %d\n", batch_serial, a.retiles);
  return true;
}

// set_plan: what was learned is only a partition of the work -- forget it and take the default rows
inline void forget_tile_rows(OrbxAdapt& a) {
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.tile_h_pref[l] = 0;
  a.prefs_applied = false;
}

// set_plan: the first pass cut unevenly (same number of tile rows, same pool), where the chooser or a forced cut says
// so.  g.bm: the band map of the tile rows in force.  first[l]: rows of tile rows 0 and 1 ({0, 0}: equal halves);
// returns whether any level has a pair.
inline bool first_pass_heights(const OrbxAdapt& a, const OrbxAdaptGeom& g, int (*first)[2]) {
  bool any = false;
  if (a.prefs_applied && a.first_split && g.top_rows == 2) {
    for (int l = 0; l < g.plan.nlevels; l++) {
      int h0 = a.cut_force[l] > 0 ? a.cut_force[l] : a.cut_pref[l];
      if (h0 <= 0 || g.bm.tiles_y[l] < 2) continue;
      const int depth = 2 * g.bm.tile_h[l], umax = fast_unit_rows_max(g.fast_impl, g.nms_radius);
      if (a.cut_force[l] > 0)  // (a forced cut goes to the nearest one the kernel can run)
        h0 = std::max(std::max(1, depth - umax), std::min(h0, std::min(umax, std::min(depth, g.plan.L[l].h) - 1)));
      first[l][0] = h0;
      first[l][1] = depth - h0;
      any = true;
    }
  }
  return any;
}

// set_plan: early bands (orbx_plan.h, pyrblur_early_rows): the rows between h0 + ORBX_TOP_MARGIN and the end of the
// first pass go to the second pass, behind a test on tile row 0 alone, on the levels where that pays by the fill rows
// the last observation window saw (early_band_pays) -- or, under a forced cut, wherever the band has three rows or
// more (tests: no histogram has been seen when their tables are built).
inline void choose_early_bands(OrbxAdapt& a, const OrbxAdaptGeom& g, FILE* trace) {
  const int top = g.top_rows;
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.early_rows[l] = 0;
  for (int l = 0; l < g.plan.nlevels; l++) {
    const int late = pyrblur_first_pass_rows(g.plan, g.bm, l, top);
    const int P = a.early_band ? pyrblur_early_rows(g.plan, g.bm, l, top, g.nms_radius) : late;
    const bool forced = a.cut_force[l] > 0;
    const bool pays = P < late && (forced ? late - P >= ORBX_PYRBLUR_EARLY_MIN_ROWS
                                          : early_band_pays(a.fill_last[l], g.bm.first_h[l][0], late - P,
                                                            pyrblur_row_cost(l, g.plan.L[l].win8)));
    a.early_rows[l] = pays ? P : late;
    if (trace && g.bm.first_h[l][0] > 0)
      fprintf(trace, "orbx early band: level %d cut %d first pass ended at %d, now ends at %d, band %d rows: %s\n", l,
              g.bm.first_h[l][0], late, a.early_rows[l], late - P,
              pays ? (forced ? "split (forced cut)" : "split") : !a.early_band ? "late" : "kept");
  }
}

}  // namespace orbx_adapt
