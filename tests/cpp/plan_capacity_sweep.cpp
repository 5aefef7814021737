// plan_capacity_sweep.cpp -- host-only sweep over (maximum, frame, tile-row preference) triples: every table a
// frame needs must fit the pool a context created for the maximum allocates, or the frame must be rejected for a
// reason that has nothing to do with the maximum.  Calls the code the library itself runs (csrc/orbx_tables.h:
// plan_with_taps; csrc/orbx_plan.h: make_bandmap, the table builders, table_capacity).  Test infrastructure only.
//
//   plan_capacity_sweep [--maxima N] [--threads T] [--parent-sizing]
//
// --parent-sizing replaces the FAST pool's capacity by what orbx_create computed before the true upper bound: the
// table of the maximum itself with ORBX_MIN_TILE_H preferred on every level.  The sweep must then FAIL (a frame
// slightly smaller than the maximum can need more); tests/test_plan_capacity.py checks that it does.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_tables.h"

using namespace orbx_tables;

namespace {

struct Config {
  int fast_impl, nlevels, nms_window;
  float scale;
};

struct Tally {
  long long maxima = 0, maxima_rejected = 0, frames = 0, frames_rejected = 0, triples = 0, failures = 0;
  std::vector<std::string> lines;  // the first failures, as printed
};

bool g_parent_sizing = false;

orbx_params params_for(const Config& c, int W, int H) {
  orbx_params p{};
  p.nfeatures = 1000;
  p.scale_factor = c.scale;
  p.nlevels = c.nlevels;
  p.threshold = 20;
  p.n = 9;
  p.nms_window = c.nms_window;
  p.patch_size = 31;
  p.harris_window = 7;
  p.harris_k = 0.04f;
  p.select_mode = ORBX_SELECT_HARRIS;
  p.blur_levels = ORBX_BLUR_ALL;
  p.blur_kind = ORBX_BLUR_SEP16;
  p.max_width = W;
  p.max_height = H;
  p.max_batch = 1;
  return p;
}

std::string pref_name(const int* pref, int nlevels) {
  if (!pref) return "none";
  std::string s = "[";
  for (int l = 0; l < nlevels; l++) s += (l ? "," : "") + std::to_string(pref[l]);
  return s + "]";
}

// one maximum under one configuration: every frame of `frames` under every preference
void sweep_one(const Config& cfg, int W, int H, const std::vector<std::pair<int, int>>& frames, std::mt19937& rng,
               Tally* t) {
  const orbx_params p = params_for(cfg, W, H);
  const int r = cfg.nms_window / 2;
  const bool strips = cfg.fast_impl == 4;
  std::string why;
  OrbxPlan M;
  OrbxTableCapacity cap2{}, cap3{};  // stand-alone blur kernel 2 (k_blur3, the default) and 3 (k_blur4)
  t->maxima++;
  if (build_plan(p, W, H, &M, &why, cfg.fast_impl) != ORBX_OK ||
      table_capacity(p, M, cfg.fast_impl, 2, &cap2, &why) != ORBX_OK ||
      table_capacity(p, M, cfg.fast_impl, 3, &cap3, &why) != ORBX_OK) {
    t->maxima_rejected++;  // orbx_create fails: there is no context whose pools could be too small
    return;
  }
  if (g_parent_sizing) {
    OrbxBandMap bmm;
    int min_pref[ORBX_MAX_LEVELS];
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) min_pref[l] = ORBX_MIN_TILE_H;
    if (make_bandmap(M, r, &bmm, &why, strips, min_pref) != ORBX_OK) {
      t->maxima_rejected++;
      return;
    }
    cap2.fast = cap3.fast = (size_t)bmm.band_begin[bmm.nbands];
  }
  char head[160];
  auto fail = [&](int w, int h, const int* pref, const char* what, size_t need, size_t have) {
    t->failures++;
    if (t->lines.size() < 8) {
      std::snprintf(head, sizeof(head), "FAIL fast_impl=%d nlevels=%d scale=%.1f nms=%d max=%dx%d frame=%dx%d pref=",
                    cfg.fast_impl, cfg.nlevels, (double)cfg.scale, cfg.nms_window, W, H, w, h);
      t->lines.push_back(std::string(head) + pref_name(pref, cfg.nlevels) + ": " + what + " needs " +
                         std::to_string(need) + ", pool holds " + std::to_string(have));
    }
  };
  const int dflt = orbx_fast3_tile_h(r);
  std::vector<OrbxResizeTap> taps;
  std::uniform_int_distribution<int> any_pref(0, dflt + 12);
  for (const auto& wh : frames) {
    const int w = wh.first, h = wh.second;
    t->frames++;
    OrbxPlan P;
    OrbxBandMap bm0;
    // a frame the library refuses whatever the context's maximum is: a level below 8 x 8, a cap above
    // ORBX_MAX_SELECT, more default tile rows than ORBX_MAX_BANDS (none of these looks at M).  P is the plan the
    // library runs, with the resize modes its taps give the levels (win8).
    if (plan_with_taps(p, w, h, cfg.fast_impl, &P, &taps, &why) != ORBX_OK || make_bandmap(P, r, &bm0, &why, strips, nullptr) != ORBX_OK) {
      t->frames_rejected++;
      continue;
    }
    // the working pools, sized per frame from M
    if (P.frame_bytes > M.frame_bytes) fail(w, h, nullptr, "pyramid frame (bytes)", P.frame_bytes, M.frame_bytes);
    if (P.mask_words > M.mask_words) fail(w, h, nullptr, "survivor mask (words)", P.mask_words, M.mask_words);
    if (P.cand_total > M.cand_total) fail(w, h, nullptr, "candidate slots", P.cand_total, M.cand_total);
    if (P.out_cap > M.out_cap) fail(w, h, nullptr, "result slots", P.out_cap, M.out_cap);
    // the tables that do not depend on the tile-row preferences
    size_t n;
    if ((n = taps_count(P)) > cap2.taps) fail(w, h, nullptr, "resize-tap table", n, cap2.taps);
    if (taps.size() != n) fail(w, h, nullptr, "resize-tap table (built)", taps.size(), n);
    if ((n = blur_tiles_for_impl(2, P, nullptr)) > cap2.frame) fail(w, h, nullptr, "blur strip table (k_blur3)", n, cap2.frame);
    if ((n = blur_tiles_for_impl(3, P, nullptr)) > cap3.frame) fail(w, h, nullptr, "blur strip table (k_blur4)", n, cap3.frame);
    // The tables that read win8, each under the plan the library runs and under the same plan with win8 zeroed, which
    // is what table_capacity sees of the maximum: 16-row pyramid tiles on every level above 0, claimed to be the most
    // tiles any win8 assignment gives -- so the real count must not exceed the zeroed one, for any table.
    OrbxPlan Z = P;
    for (int l = 0; l < Z.nlevels; l++) Z.L[l].win8 = 0;
    size_t nz;
    if ((nz = build_frame_tiles(Z, ORBX_PYR2_TW, ORBX_PYR2_TH, true, nullptr)) > std::min(cap2.frame, cap3.frame))
      fail(w, h, nullptr, "pyramid tile table", nz, std::min(cap2.frame, cap3.frame));
    if ((n = build_frame_tiles(P, ORBX_PYR2_TW, ORBX_PYR2_TH, true, nullptr)) > std::min(cap2.frame, cap3.frame))
      fail(w, h, nullptr, "pyramid tile table (real win8)", n, std::min(cap2.frame, cap3.frame));
    if (n > nz) fail(w, h, nullptr, "pyramid tile table: real win8 against win8 zeroed", n, nz);
    if ((nz = build_pyrblur_tiles(Z, ORBX_PYRBLUR_RH, nullptr)) > std::min(cap2.frame, cap3.frame))
      fail(w, h, nullptr, "pyramid+blur strip table", nz, std::min(cap2.frame, cap3.frame));
    if ((n = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, nullptr)) > std::min(cap2.frame, cap3.frame))
      fail(w, h, nullptr, "pyramid+blur strip table (real win8)", n, std::min(cap2.frame, cap3.frame));
    if (n > nz) fail(w, h, nullptr, "pyramid+blur strip table: real win8 against win8 zeroed", n, nz);
    if ((nz = build_pyrblur_tiles(Z, ORBX_PYRBLUR_RH_SMALL, nullptr)) > cap2.small)
      fail(w, h, nullptr, "pyramid+blur short-band table", nz, cap2.small);
    if ((n = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH_SMALL, nullptr)) > cap2.small)
      fail(w, h, nullptr, "pyramid+blur short-band table (real win8)", n, cap2.small);
    if (n > nz) fail(w, h, nullptr, "pyramid+blur short-band table: real win8 against win8 zeroed", n, nz);
    // tile-row preferences: none, every uniform value, random per-level vectors
    int pref[ORBX_MAX_LEVELS];
    const int nuniform = dflt - ORBX_MIN_TILE_H + 1, nrandom = 6;
    for (int k = -1; k < nuniform + nrandom; k++) {
      const int* pp = nullptr;
      if (k >= 0) {
        for (int l = 0; l < ORBX_MAX_LEVELS; l++) pref[l] = k < nuniform ? ORBX_MIN_TILE_H + k : any_pref(rng);
        pp = pref;
      }
      t->triples++;
      OrbxBandMap bm;
      if (make_bandmap(P, r, &bm, &why, strips, pp) != ORBX_OK) {
        // the default rows were accepted above: a preference must not make the frame unusable
        fail(w, h, pp, ("FAST tile table refused (" + why + "); tile rows").c_str(), 0, ORBX_MAX_BANDS);
        continue;
      }
      const size_t nf = (size_t)bm.band_begin[bm.nbands];
      if (nf > cap2.fast) fail(w, h, pp, "FAST tile table", nf, cap2.fast);
      // the split tables of the top-rows-first pipeline follow the FAST tile rows; and the count the band map
      // gives is the count of the table build_fast_tiles writes (checked where the tables are built anyway)
      if (k == -1 || k == 0 || k == nuniform - 1 || k >= nuniform + nrandom - 2) {
        if (build_fast_tiles(P, bm, 0, 1, nullptr) != nf) fail(w, h, pp, "FAST tile table (built)", build_fast_tiles(P, bm, 0, 1, nullptr), nf);
        for (int top = 1; top <= 3; top++)
          for (int part = 1; part <= 2; part++)
            if ((n = build_pyrblur_tiles(P, ORBX_PYRBLUR_RH, nullptr, false, part, &bm, top)) > std::min(cap2.frame, cap3.frame))
              fail(w, h, pp, part == 1 ? "first-pass strip table" : "second-pass strip table", n, std::min(cap2.frame, cap3.frame));
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  int nrandom_maxima = 200, nthreads = 0;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--parent-sizing")
      g_parent_sizing = true;
    else if (a == "--maxima" && i + 1 < argc)
      nrandom_maxima = std::atoi(argv[++i]);
    else if (a == "--threads" && i + 1 < argc)
      nthreads = std::atoi(argv[++i]);
    else {
      std::fprintf(stderr, "usage: %s [--maxima N] [--threads T] [--parent-sizing]\n", argv[0]);
      return 2;
    }
  }
  if (nthreads <= 0) nthreads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));

  std::vector<std::pair<int, int>> maxima = {{600, 1100}, {2191, 2141}, {1080, 1920}, {1920, 1200}, {1241, 376}, {800, 1280}};
  {
    std::mt19937 rng(20240611u);
    std::uniform_int_distribution<int> side(64, 4096);
    for (int i = 0; i < nrandom_maxima; i++) {
      const int W = side(rng), H = side(rng);
      maxima.push_back({W, H});
    }
  }
  std::vector<Config> configs;
  for (int impl : {4, 3})
    for (int nl : {8, 12})
      for (float sf : {1.2f, 1.5f})
        for (int nms : {3, 7}) configs.push_back(Config{impl, nl, nms, sf});

  Tally total;
  std::mutex mu;
  std::atomic<size_t> next{0};
  auto worker = [&]() {
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= maxima.size()) return;
      const int W = maxima[i].first, H = maxima[i].second;
      std::mt19937 rng(977u * (unsigned)i + 13u);  // (per maximum: the result does not depend on the thread count)
      // every frame within 96 rows and 8 columns below the maximum, and a random sample of smaller ones
      std::vector<std::pair<int, int>> frames;
      for (int h = std::max(8, H - 96); h <= H; h++)
        for (int w = std::max(8, W - 8); w <= W; w++) frames.push_back({w, h});
      std::uniform_int_distribution<int> rw(8, W), rh(8, H);
      for (int k = 0; k < 24; k++) frames.push_back({rw(rng), rh(rng)});
      Tally t;
      for (const Config& c : configs) sweep_one(c, W, H, frames, rng, &t);
      std::lock_guard<std::mutex> lock(mu);
      total.maxima += t.maxima;
      total.maxima_rejected += t.maxima_rejected;
      total.frames += t.frames;
      total.frames_rejected += t.frames_rejected;
      total.triples += t.triples;
      total.failures += t.failures;
      for (const std::string& s : t.lines)
        if (total.lines.size() < 400) total.lines.push_back(s);
    }
  };
  std::vector<std::thread> pool;
  for (int k = 0; k < nthreads; k++) pool.emplace_back(worker);
  for (std::thread& th : pool) th.join();

  for (const std::string& s : total.lines) std::printf("%s\n", s.c_str());
  std::printf("plan_capacity_sweep%s: %lld (maximum, configuration) pairs (%lld not creatable), %lld frames (%lld refused "
              "whatever the maximum), %lld (maximum, frame, preference) triples, %lld failures\n",
              g_parent_sizing ? " [parent sizing]" : "", total.maxima, total.maxima_rejected, total.frames,
              total.frames_rejected, total.triples, total.failures);
  return total.failures ? 1 : 0;
}
