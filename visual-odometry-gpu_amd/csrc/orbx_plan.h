// orbx_plan.h -- the geometry of a frame size: level sizes, the per-frame layout of the working pools, the tile /
// strip tables of the kernels and the capacities a context sizes its table pools with.  Host arithmetic only, no
// HIP in it: orbx_api.cpp runs this code, and tests/cpp/plan_capacity_sweep.cpp calls the very same functions to
// check that every frame a context accepts fits the pools its maximum provides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbx.h"

// ---- HBM layout ------------------------------------------------------------
// A "pyramid frame" holds all levels of one input frame back to back:
//   level l at byte offset img_off, `h` rows of `pitch` bytes, pitch = W_l
//   rounded up to 64 (so every tile row starts 4-byte aligned and a 64-pixel
//   tile row never straddles the allocation), level offsets 256-B aligned.
// The NMS survivor mask of a level is h rows of `mask_wpr` 64-bit words
// (bit x&63 of word x>>6), all levels back to back at mask_off (in words).
// Candidate keypoints / Harris responses of a frame live in `cand_total`
// slots, level l owning [cand_off, cand_off + cap).
struct OrbxLevel {
  int32_t w, h, pitch;
  int32_t img_off;   // bytes, within a pyramid frame
  int32_t mask_wpr;  // u64 words per mask row
  int32_t mask_off;  // u64 words, within a frame's mask block
  int32_t cap;       // FAST cap (row-major)        src/orb.cpp:63
  int32_t quota;     // kept after selection        src/orb.cpp:62
  int32_t cand_off;  // first candidate slot
  int32_t xtab_off;  // first entry of this level's resize x-table
  int32_t ytab_off;  // first entry of this level's resize y-table
  float scale;       // (float)pow(scaleFactor, l)  src/orb.cpp:95
  int32_t out_off;   // first STATIC selection slot of this level = sum of the lower levels' quotas
  int32_t win8;      // resize: 1: the 4 source pairs of any aligned group of 4 outputs fit one 8-byte window; 3: a strip's source span fits the LDS staging rows of k_pyrblur; 0: neither (2-byte gathers)
  // 0: classic mask rows (bit x & 63 of word x >> 6).  > 0: STRIP layout of the streaming FAST kernel
  // (orbx_fast4.hip): 4 words per strip and row, word 4 s + q of a row holds pixels mask_strip_px * s + 64 q + bit
  // (a strip's first / last halo pixels are zero bits), so x = (xw >> 2) * mask_strip_px + (xw & 3) * 64 + bit
  int32_t mask_strip_px;
};

struct OrbxPlan {
  int32_t nlevels;
  int32_t w0, h0;
  int32_t frame_bytes;  // pyramid frame stride (bytes)
  int32_t mask_words;   // mask stride per frame (u64 words)
  int32_t cand_total;   // candidate slots per frame
  int32_t out_cap;      // result slots per frame (sum of quotas)
  OrbxLevel L[ORBX_MAX_LEVELS];
};

// blockIdx.x -> (level, tile) map for one kernel's tile size
struct OrbxTileMap {
  int32_t begin[ORBX_MAX_LEVELS + 1];  // first tile id of each level (+ total)
  int32_t tiles_x[ORBX_MAX_LEVELS];
};

// band-major workgroup order of the FAST kernel (see decode_band)
#define ORBX_MAX_BANDS 64
// smallest FAST tile-row height the adaptive first pass may choose (orbx_adapt.h, adapt_tile_rows)
#define ORBX_MIN_TILE_H 16
// most rows a unit of the streaming FAST kernel may have: the tags of its score rows repeat after lcm(7 + 2 R, 16)
// >= 144 rows (orbx_fast4.hip); a tile of the LDS tile kernel holds orbx_fast3_tile_h(R) rows
#define ORBX_FAST_UNIT_ROWS_MAX 128
struct OrbxBandMap {
  int32_t nbands;
  int32_t band_begin[ORBX_MAX_BANDS + 1];  // tiles PER FRAME before band b (+ total)
  int32_t tiles_x[ORBX_MAX_LEVELS];
  int32_t tiles_y[ORBX_MAX_LEVELS];
  int32_t tile_h[ORBX_MAX_LEVELS];       // rows per FAST tile of the level (balanced: ceil(h / tiles_y))
  int32_t xprefix[ORBX_MAX_LEVELS + 1];  // prefix sums of tiles_x
  // unevenly cut first pass (make_bandmap, first_h): rows of tile rows 0 and 1 of the level, together 2 * tile_h;
  // {0, 0}: every tile row has tile_h rows
  int32_t first_h[ORBX_MAX_LEVELS][2];
};

// One 64-byte record per workgroup, read with a single scalar load: everything a
// tile kernel needs to know about its tile.  Replaces the chains of dependent
// scalar loads that decoding blockIdx through the plan / tile maps costs at the
// start of every wave (~20 s_load round trips for the FAST kernel).
//   FAST table   : one entry per (tile row, level, tx) of ONE frame in band-major order
//                  (grid = frames x tiles, frame index dispatched fastest); `f` = rows per tile
//                  of this level, `pad` = the unit's own rows: first row | rows << 16 (the two
//                  tile rows of an unevenly cut first pass differ from ty * f and f).
//   pyramid      : one entry per (level, tx, ty) of ONE frame (blockIdx.y = frame); u0/u1/u2
//                  carry xtab_off / ytab_off / win8 and `f` the rows per wave.
//   blur         : one entry per (level, 256-px strip, row band): tx = strip, ty = first row,
//                  f = rows of the band.
//                  fused pyramid + blur, second pass of the top-rows-first pipeline: stat_index = first
//                  tile-row statistic of the level, mask_off = (FAST tile rows of the first pass) << 32 | cap,
//                  bit 62 set in ONE strip per frame (its wave reports how many levels of the frame were skipped).
//   img_off / mask_off are offsets inside one frame's pyramid / mask block.
struct OrbxTileDesc {
  int32_t l, tx, ty, f;
  int32_t w, h, pitch;
  int32_t u0;  // FAST: cap            pyramid: xtab_off
  int32_t u1;  // FAST: mask_wpr       pyramid: ytab_off
  int32_t u2;  // FAST: tiles_x        pyramid: win8
  uint32_t stat_index;  // FAST: first tile-row statistic of (frame, level)
  uint32_t pad;         // FAST: first row | rows << 16 of the unit   fused pyramid + blur: strips of the level
  uint64_t img_off;   // bytes from the pyramid base
  uint64_t mask_off;  // u64 words from the mask base (FAST)
};
static_assert(sizeof(OrbxTileDesc) == 64, "one 64-byte scalar load per workgroup");

// 8-bit bilinear resize coefficient (OpenCV-style 11-bit fixed point)
struct OrbxResizeTap {
  int32_t ofs;     // source index (clamped)
  int16_t c0, c1;  // weights of src[ofs], src[ofs+1]; c0+c1 ~ 2048
};

// the levels whose lower rows the second pass of the top-rows-first pipeline may skip (orbx_api.cpp, enqueue_batch)
struct OrbxTopLevels {
  int32_t n;
  int32_t stat_index[ORBX_MAX_LEVELS];  // first tile-row statistic of the level
  int32_t rows[ORBX_MAX_LEVELS];        // FAST tile rows of the first pass
  int32_t cap[ORBX_MAX_LEVELS];
};

// tile geometry of the FAST/NMS kernel (orbx_fast.hip): 128 output pixels wide (two mask words per
// row); 34 dword columns x 7 row segments of walking threads, 7 rows per walk (at most 8: a flag byte per
// pixel column), so the score region of a tile has 49 rows and a tile 49 - 2 * nms_radius output rows
#define ORBX_FAST3_TW 128
#define ORBX_FAST3_K 7
constexpr int orbx_fast3_tile_h(int nms_radius) {
  return (256 / (ORBX_FAST3_TW / 4 + 2)) * ORBX_FAST3_K - 2 * nms_radius;
}
// streaming FAST kernel (orbx_fast4.hip): a wave owns a strip of 64 dwords; the outer `halo` dwords of a side are
// context for the ring (3 px) and the NMS window (R px) of the pixels next to them; tile rows as above
constexpr int orbx_fast4_halo(int nms_radius) { return (nms_radius + 3 + 3) / 4; }
constexpr int orbx_fast4_strip_lanes(int nms_radius) { return 64 - 2 * orbx_fast4_halo(nms_radius); }
constexpr int orbx_fast4_strips(int w, int nms_radius) {
  const int ndw = (w + 3) / 4, s = orbx_fast4_strip_lanes(nms_radius), n = (ndw - 2 * orbx_fast4_halo(nms_radius) + s - 1) / s;
  return n < 1 ? 1 : n;
}
// tile geometry of the blur kernel
#define ORBX_BLUR_TW 64
#define ORBX_BLUR_TH 16
// register-streaming separable blur (orbx_blur.hip): a wave owns a strip of 256 pixels (one aligned
// 256-byte segment per row) over a band of at most ORBX_BLUR3_RH rows
#define ORBX_BLUR3_TW 256
#define ORBX_BLUR3_RH 64
// k_blur4: 16 pixels per lane, a wave = a 256-px strip x 4 row bands of at most ORBX_BLUR4_RH rows
#define ORBX_BLUR4_TW 256
#define ORBX_BLUR4_RH 96
// fused pyramid + blur: the halo dwords are computed, not loaded, so lanes 0 / 63 are halo-only
#define ORBX_PYRBLUR_TW 248
// LDS staging of the source rows of the levels whose pairs do not fit the 8-byte window (scale > 2): bytes of a
// source row a strip may need.  (Measured per level of 1241x376, 256 frames: scale 2.1: 41 us staged / 56 us with
// 2-byte gathers, 2.5: 35 / 43, 3.0: 27 / 32, 3.5 (896 bytes): 30 / 29 -- the staged loads cost the texture
// addresser a cycle per four lane-dwords like any other, and at 8 x 104 bytes they are as many as the gathers'.)
#define ORBX_PYR_STAGE_BYTES 832
// rows per band of the fused kernel: the y taps of a band's input rows (rows + 6) sit one per lane
#define ORBX_PYRBLUR_RH 58
#define ORBX_PYRBLUR_RH_SMALL 12  // few frames per call: many short waves instead
// pyramid kernel: a wave owns 256 x 8 pixels (level 0 and the levels resized through 8-byte
// windows) or 256 x 4, a workgroup four times that; OrbxTileDesc::f carries the rows per wave
#define ORBX_PYR2_TW 256
#define ORBX_PYR2_TH 16  // smallest tile height (sizes the tile table pool)

#define ORBX_MAX_SELECT 4096  // largest per-level FAST cap the selection kernel holds in LDS (16 B per candidate)

// a descriptor reaches DESC_R = 20 rows below its keypoint (orbx_kernels.hip); Harris, FAST less
#define ORBX_TOP_MARGIN 21

namespace orbx_geom {

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }
inline size_t align_up_sz(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- geometry (src/orb.cpp:62, :95, :117-118) ------------------------------

inline float level_scale(float sf, int l) { return (float)std::pow((double)sf, (double)l); }

inline void level_size(int w0, int h0, float sf, int l, int* wl, int* hl) {
  if (l == 0) {
    *wl = w0;
    *hl = h0;
    return;
  }
  const float scale = level_scale(sf, l);
  *wl = (int)std::round((double)((float)w0 / scale));
  *hl = (int)std::round((double)((float)h0 / scale));
}

inline int level_quota(int nfeatures, float sf, int nlevels, int l) {
  // int * ((float - float) / (int - double)) * double, truncated to int
  const float inv = 1 / sf;
  const float num = 1 - inv;
  const double den = 1 - std::pow((double)inv, (double)nlevels);
  return (int)(nfeatures * ((double)num / den) * std::pow((double)inv, (double)l));
}

inline void make_tilemap(const OrbxPlan& plan, int tw, int th, bool use_pitch, OrbxTileMap* tm) {
  int acc = 0;
  for (int l = 0; l < plan.nlevels; l++) {
    const int wcols = use_pitch ? plan.L[l].pitch : plan.L[l].w;
    const int tx = (wcols + tw - 1) / tw, ty = (plan.L[l].h + th - 1) / th;
    tm->begin[l] = acc;
    tm->tiles_x[l] = tx;
    acc += tx * ty;
  }
  for (int l = plan.nlevels; l <= ORBX_MAX_LEVELS; l++) tm->begin[l] = acc;
}

// units per tile row of a level: strips of the streaming kernel of the whole path (orbx_fast4.hip: a wave per
// 64-dword strip and tile row) or the 128-pixel tiles of the LDS tile kernel (stage operators)
inline int fast_tiles_x(int w, int nms_radius, bool strips) {
  return strips ? orbx_fast4_strips(w, nms_radius) : (w + ORBX_FAST3_TW - 1) / ORBX_FAST3_TW;
}

// band-major order of the FAST tiles (levels shrink with the level index, so the
// levels that have a tile row b are always a prefix of the level list)
// first_h[l] = {rows of tile row 0, rows of tile row 1}: the two tile rows of the first pass of the top-rows-first
// pipeline cut UNEVENLY (adapt_tile_rows: tile row 0 ends where most frames have filled their cap, and the units of
// the short tile row 1 exit for those frames).  The pair must keep the depth of the first pass, 2 * tile_h, so
// that the tile rows below and their number stay what they are; a pair that does not, that leaves a unit more rows
// than its kernel holds, or whose tile row 0 swallows the level is ignored (equal tile rows).
inline int make_bandmap(const OrbxPlan& plan, int nms_radius, OrbxBandMap* bm, std::string* why, bool strips = false,
                        const int* pref_h = nullptr, const int (*first_h)[2] = nullptr) {
  std::memset(bm, 0, sizeof(*bm));
  const int th = orbx_fast3_tile_h(nms_radius);
  int nb = 0;
  for (int l = 0; l < plan.nlevels; l++) {
    bm->tiles_x[l] = fast_tiles_x(plan.L[l].w, nms_radius, strips);
    bm->tiles_y[l] = (plan.L[l].h + th - 1) / th;
    bm->tile_h[l] = (plan.L[l].h + bm->tiles_y[l] - 1) / bm->tiles_y[l];  // balanced tile rows
    // pref_h[l] > 0: SHORTER tile rows for this level (the adaptive first pass of the top-rows-first pipeline:
    // adapt_tile_rows) -- never more tile rows than ORBX_MAX_BANDS or than the level above has (band-major order)
    if (pref_h && pref_h[l] > 0 && pref_h[l] < bm->tile_h[l]) {
      int hh = std::max(pref_h[l], ORBX_MIN_TILE_H);
      const int most = l > 0 ? std::min(bm->tiles_y[l - 1], ORBX_MAX_BANDS) : ORBX_MAX_BANDS;
      while ((plan.L[l].h + hh - 1) / hh > most) hh++;
      if (hh < bm->tile_h[l]) {
        bm->tile_h[l] = hh;
        bm->tiles_y[l] = (plan.L[l].h + hh - 1) / hh;
      }
    }
    if (first_h && first_h[l][0] > 0 && first_h[l][1] > 0) {
      const int a = first_h[l][0], b = first_h[l][1];
      const int unit_max = strips ? ORBX_FAST_UNIT_ROWS_MAX : th;
      if (a + b == 2 * bm->tile_h[l] && bm->tiles_y[l] >= 2 && a < plan.L[l].h && a <= unit_max && b <= unit_max) {
        bm->first_h[l][0] = a;
        bm->first_h[l][1] = b;
      }
    }
    bm->xprefix[l + 1] = bm->xprefix[l] + bm->tiles_x[l];
    if (l > 0 && bm->tiles_y[l] > bm->tiles_y[l - 1]) {
      *why = "pyramid levels must not grow with the level index";
      return ORBX_ERR_UNSUPPORTED;
    }
    nb = std::max(nb, bm->tiles_y[l]);
  }
  if (nb > ORBX_MAX_BANDS) {
    *why = "image taller than ORBX_MAX_BANDS FAST tile rows";
    return ORBX_ERR_UNSUPPORTED;
  }
  bm->nbands = nb;
  int acc = 0;
  for (int b = 0; b < nb; b++) {
    bm->band_begin[b] = acc;
    for (int l = 0; l < plan.nlevels; l++)
      if (bm->tiles_y[l] > b) acc += bm->tiles_x[l];
  }
  for (int b = nb; b <= ORBX_MAX_BANDS; b++) bm->band_begin[b] = acc;
  return ORBX_OK;
}

// first row and rows of tile row b of a level (the last tile row may reach past the level's height: the kernels clip)
inline void fast_band_rows(const OrbxBandMap& bm, int l, int b, int* y0, int* rows) {
  const bool cut = bm.first_h[l][0] > 0 && b < 2;
  *y0 = cut ? (b == 0 ? 0 : bm.first_h[l][0]) : b * bm.tile_h[l];
  *rows = cut ? bm.first_h[l][b] : bm.tile_h[l];
}

// The table builders below return the number of entries and fill `out` unless it is NULL (count only).

// FAST tiles of ONE frame in band-major order (the kernel's grid is frames x tiles with
// the frame index dispatched fastest, so tile row b of every frame runs before tile row
// b+1 of any frame).  Tile rows >= first_band only; a workgroup owns `strip` tiles of a row.
inline size_t build_fast_tiles(const OrbxPlan& plan, const OrbxBandMap& bm, int first_band, int strip,
                               std::vector<OrbxTileDesc>* out) {
  size_t cnt = 0;
  if (out) out->clear();
  for (int b = first_band; b < bm.nbands; b++)
    for (int l = 0; l < plan.nlevels; l++) {
      if (bm.tiles_y[l] <= b) continue;
      const OrbxLevel& L = plan.L[l];
      int y0, rows;
      fast_band_rows(bm, l, b, &y0, &rows);
      for (int tx = 0; tx < bm.tiles_x[l]; tx += strip) {
        OrbxTileDesc d{};
        d.l = l;
        d.tx = tx;
        d.ty = b;
        d.f = bm.tile_h[l];
        d.pad = (uint32_t)y0 | ((uint32_t)rows << 16);
        d.w = L.w;
        d.h = L.h;
        d.pitch = L.pitch;
        d.u0 = L.cap;
        d.u1 = L.mask_wpr;
        d.u2 = bm.tiles_x[l];
        d.stat_index = (uint32_t)(l * ORBX_MAX_BANDS);
        d.img_off = (uint64_t)L.img_off;
        d.mask_off = (uint64_t)L.mask_off;
        if (out) out->push_back(d);
        cnt++;
      }
    }
  return cnt;
}

// tiles of ONE frame, level-major, for the blur / pyramid kernels (blockIdx.y = frame)
inline size_t build_frame_tiles(const OrbxPlan& plan, int tw, int th, bool pyramid_fields, std::vector<OrbxTileDesc>* out) {
  size_t cnt = 0;
  if (out) out->clear();
  for (int l = 0; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    // pyramid tiles: 8 rows per wave where a lane keeps only 4 registers per row in flight
    // (level 0 copy, 8-byte-window levels), else 4
    const int rpw = pyramid_fields ? ((l == 0 || L.win8 == 1) ? 8 : 4) : 0;
    if (pyramid_fields) th = 4 * rpw;
    const int ntx = (L.pitch + tw - 1) / tw, nty = (L.h + th - 1) / th;
    for (int ty = 0; ty < nty; ty++)
      for (int tx = 0; tx < ntx; tx++) {
        OrbxTileDesc d{};
        d.l = l;
        d.tx = tx;
        d.ty = ty;
        d.f = rpw;
        d.w = L.w;
        d.h = L.h;
        d.pitch = L.pitch;
        if (pyramid_fields) {
          d.u0 = L.xtab_off;
          d.u1 = L.ytab_off;
          d.u2 = L.win8 == 1;  // (k_pyramid2 knows the one-window mode only)
        }
        d.img_off = (uint64_t)L.img_off;
        if (out) out->push_back(d);
        cnt++;
      }
  }
  return cnt;
}

// strips of the streaming blur for ONE frame: per level ceil(pitch / 256) strips x balanced row bands of
// at most ORBX_BLUR3_RH rows (one wave each; the 4 warm-up rows of the vertical pass are per band)
inline size_t build_blur_tiles(const OrbxPlan& plan, std::vector<OrbxTileDesc>* out) {
  size_t cnt = 0;
  if (out) out->clear();
  for (int l = 0; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    const int ntx = (L.pitch + ORBX_BLUR3_TW - 1) / ORBX_BLUR3_TW;  // the padding bytes are (re)written as zeros
    const int nb = (L.h + ORBX_BLUR3_RH - 1) / ORBX_BLUR3_RH, rows = (L.h + nb - 1) / nb;
    for (int b = 0; b < nb; b++)
      for (int tx = 0; tx < ntx; tx++) {
        OrbxTileDesc d{};
        d.l = l;
        d.tx = tx;
        d.ty = b * rows;
        d.f = std::min(rows, L.h - b * rows);
        d.w = L.w;
        d.h = L.h;
        d.pitch = L.pitch;
        d.img_off = (uint64_t)L.img_off;
        if (d.f > 0) {
          if (out) out->push_back(d);
          cnt++;
        }
      }
  }
  return cnt;
}

// units of k_blur4 for ONE frame: per level ceil(pitch / 256) strips x waves of FOUR row bands each (f = rows per
// band: a level's height spread over the fewest waves whose bands stay within ORBX_BLUR4_RH rows)
inline size_t build_blur4_tiles(const OrbxPlan& plan, std::vector<OrbxTileDesc>* out) {
  size_t cnt = 0;
  if (out) out->clear();
  for (int l = 0; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    const int ntx = (L.pitch + ORBX_BLUR4_TW - 1) / ORBX_BLUR4_TW;  // the padding bytes are (re)written as zeros
    const int nwv = (L.h + 4 * ORBX_BLUR4_RH - 1) / (4 * ORBX_BLUR4_RH), rows = (L.h + 4 * nwv - 1) / (4 * nwv);
    for (int wv = 0; wv < nwv; wv++)
      for (int tx = 0; tx < ntx; tx++) {
        OrbxTileDesc d{};
        d.l = l;
        d.tx = tx;
        d.ty = wv * 4 * rows;
        d.f = rows;
        d.w = L.w;
        d.h = L.h;
        d.pitch = L.pitch;
        d.img_off = (uint64_t)L.img_off;
        if (d.ty < L.h) {
          if (out) out->push_back(d);
          cnt++;
        }
      }
  }
  return cnt;
}

// the strip table of the stand-alone blur is built for the kernel that reads it (ORBX_BLUR_IMPL: 3 = k_blur4)
inline size_t blur_tiles_for_impl(int impl, const OrbxPlan& plan, std::vector<OrbxTileDesc>* out) {
  return impl == 3 ? build_blur4_tiles(plan, out) : build_blur_tiles(plan, out);
}

// strips of the fused pyramid + blur kernel for ONE frame: 248-px strips (the halo dwords are
// computed by lanes 0 / 63) x balanced row bands, with the level's resize-table fields.
// part 0: every row.  Top-rows-first pipeline (enqueue_batch): part 1 = the rows the FAST tiles of the
// first `top_rows` tile rows and the descriptors of their keypoints can read -- the rows above the end of the
// last of those tile rows + ORBX_TOP_MARGIN -- and part 2 = the rest, whose strips carry what the kernel's skip
// test needs (stat_index, mask_off = tile rows of the first pass << 32 | cap).
inline int pyrblur_first_pass_rows(const OrbxPlan& plan, const OrbxBandMap& bm, int l, int top_rows) {
  if (top_rows <= 0 || bm.tiles_y[l] <= top_rows) return plan.L[l].h;
  int y0, rows;
  fast_band_rows(bm, l, top_rows - 1, &y0, &rows);
  return std::min(plan.L[l].h, y0 + rows + ORBX_TOP_MARGIN);
}
//
// The early band.  With the first pass cut unevenly (make_bandmap, first_h) tile row 0 of a level ends at h0, where
// most frames have filled their cap: such a frame has every keypoint in rows < h0, and nothing of it reads a row at
// or below h0 + ORBX_TOP_MARGIN.  The FAST units of the first launch (tile rows 0 and 1) read up to the end of tile
// row 1, D, plus their context: a pixel's ring reaches 3 rows and the NMS window R rows below a unit's last row, so
// R + 3 rows for the streaming kernel (orbx_fast4.hip) and for the LDS tile kernel alike (orbx_fast.hip loads its
// whole LDS tile, more rows than that, but looks at nothing below the unit's rows + R + 3).  So the rows
// [P, D + ORBX_TOP_MARGIN) with P = max(h0 + ORBX_TOP_MARGIN, D + R + 3) are read only for the frames that did not
// fill in tile row 0: they can go to the second pass as strips of their own whose skip test looks at tile row 0
// alone (na = 1).  pyrblur_early_rows: P of a level, or the end of the first pass where there is no such band (no
// uneven cut, or the first pass covers the level: then the level has no second-pass strips and no verdict).
inline int pyrblur_early_rows(const OrbxPlan& plan, const OrbxBandMap& bm, int l, int top_rows, int nms_radius) {
  const int late = pyrblur_first_pass_rows(plan, bm, l, top_rows);
  if (top_rows != 2 || bm.tiles_y[l] <= top_rows || bm.first_h[l][0] <= 0 || late >= plan.L[l].h) return late;
  const int h0 = bm.first_h[l][0], D = h0 + bm.first_h[l][1];
  return std::min(late, std::max(h0 + ORBX_TOP_MARGIN, D + nms_radius + 3));
}
// strips per row band of a level: 62 dwords that hold image pixels per strip, one more in the first and in the last
// strip (their outer neighbour is a reflection, not another strip's dword).  The padding dwords beyond are not
// written by the kernel: they are zeroed when the plan is set.
inline int pyrblur_strips_x(int w) {
  const int dw = (w + 3) / 4;
  return dw <= 64 ? 1 : (dw - 2 + 61) / 62;
}
// estimated instructions per strip row: level 0 copies, the 8-byte-window levels resize, the others gather; a band
// pays 4 warm-up rows on top of its own
inline int pyrblur_row_cost(int l, int win8) { return l == 0 ? 35 : win8 == 1 ? 80 : 90; }
#define ORBX_PYRBLUR_WARMUP_ROWS 4
// early_rows (optional, parts 1 and 2; only set_plan passes it): per level, the row at which the first pass ends
// instead of pyrblur_first_pass_rows' (0, or anything outside (0, that row): no early band for the level).
inline size_t build_pyrblur_tiles(const OrbxPlan& plan, int max_rows, std::vector<OrbxTileDesc>* out,
                                  bool heavy_first = false, int part = 0, const OrbxBandMap* bm = nullptr,
                                  int top_rows = 0, const int* early_rows = nullptr) {
  size_t cnt = 0;
  if (out) out->clear();
  bool have_reporter = false;
  for (int l = 0; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    const int ntx = pyrblur_strips_x(L.w);
    const int split = part == 0 ? L.h : pyrblur_first_pass_rows(plan, *bm, l, top_rows);
    const int early = part != 0 && early_rows && early_rows[l] > 0 && early_rows[l] < split ? early_rows[l] : split;
    // row ranges of this part: {first row, end, tile rows of the skip test}
    const int seg[2][3] = {{part == 2 ? early : 0, part == 1 ? early : part == 2 ? split : L.h, 1},
                           {split, part == 2 ? L.h : split, std::min(top_rows, bm ? bm->tiles_y[l] : 0)}};
    for (int s = 0; s < 2; s++) {
      const int r0 = seg[s][0], r1 = seg[s][1];
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
            d.mask_off = ((uint64_t)(uint32_t)seg[s][2] << 32) | (uint32_t)L.cap;
            // this strip's wave reports the verdicts of all the frame's levels (never a strip of an early band: the
            // report comes before the strip's own test, but the levels' verdicts are those of the whole first pass)
            if (s == 1 && b == 0 && tx == 0 && !have_reporter) {
              d.mask_off |= 1ull << 62;
              have_reporter = true;
            }
          }
          if (d.f > 0) {
            if (out) out->push_back(d);
            cnt++;
          }
        }
    }
  }
  if (heavy_first && out) {
    auto cost = [](const OrbxTileDesc& d) { return (d.f + ORBX_PYRBLUR_WARMUP_ROWS) * pyrblur_row_cost(d.l, d.u2); };
    std::stable_sort(out->begin(), out->end(),
                     [&](const OrbxTileDesc& a, const OrbxTileDesc& b) { return cost(a) > cost(b); });
  }
  return cnt;
}

// fast_impl 4: the streaming FAST kernel's strip layout of the survivor masks, 3: classic mask rows
inline int build_plan(const orbx_params& p, int w0, int h0, OrbxPlan* plan, std::string* why, int fast_impl = 3) {
  std::memset(plan, 0, sizeof(*plan));
  plan->nlevels = p.nlevels;
  plan->w0 = w0;
  plan->h0 = h0;
  size_t img_off = 0, mask_off = 0;
  int cand_off = 0, out_cap = 0, xt = 0;
  for (int l = 0; l < p.nlevels; l++) {
    OrbxLevel& L = plan->L[l];
    level_size(w0, h0, p.scale_factor, l, &L.w, &L.h);
    if (L.w < 8 || L.h < 8) {
      *why = "pyramid level " + std::to_string(l) + " is smaller than 8x8 (" + std::to_string(L.w) + "x" +
             std::to_string(L.h) + ")";
      return ORBX_ERR_UNSUPPORTED;
    }
    L.pitch = align_up(L.w, 64);
    L.img_off = (int32_t)img_off;
    img_off = align_up_sz(img_off + (size_t)L.pitch * L.h, 256);
    // the whole path's FAST kernel writes its survivor masks in strip layout (orbx_fast4.hip)
    if (fast_impl == 4) {
      L.mask_strip_px = 4 * orbx_fast4_strip_lanes(p.nms_window / 2);
      L.mask_wpr = 4 * orbx_fast4_strips(L.w, p.nms_window / 2);
    } else {
      L.mask_wpr = (L.w + 63) / 64;
    }
    L.mask_off = (int32_t)mask_off;
    mask_off += (size_t)L.mask_wpr * L.h;
    int quota;
    if (p.select_mode == ORBX_SELECT_ROWMAJOR && p.nlevels == 1)
      quota = p.nfeatures;  // OrientedFASTCPU::detect cap (src/orb_cpu.cpp:110)
    else
      quota = level_quota(p.nfeatures, p.scale_factor, p.nlevels, l);
    if (quota < 0) quota = 0;
    L.quota = quota;
    L.cap = p.select_mode == ORBX_SELECT_HARRIS ? 2 * quota : quota;  // src/orb.cpp:63
    if (L.cap > ORBX_MAX_SELECT) {
      *why = "per-level FAST cap " + std::to_string(L.cap) + " exceeds ORBX_MAX_SELECT";
      return ORBX_ERR_UNSUPPORTED;
    }
    L.cand_off = cand_off;
    cand_off += L.cap;
    L.out_off = out_cap;
    out_cap += quota;
    L.scale = level_scale(p.scale_factor, l);
    // x table first (padded to a multiple of 4 entries = 32 bytes so that a thread's
    // four taps are two aligned 16-byte loads), then the y table
    L.xtab_off = xt;
    L.ytab_off = xt + (l == 0 ? 0 : align_up(L.w, 4));
    xt += (l == 0 ? 0 : align_up(L.w, 4) + align_up(L.h, 4));
    if (img_off > 0x7fffffffull) {
      *why = "pyramid frame exceeds 2 GiB";
      return ORBX_ERR_UNSUPPORTED;
    }
  }
  plan->frame_bytes = (int32_t)img_off;
  plan->mask_words = (int32_t)mask_off;
  // (the selection output lives in the candidate pools, at the result blocks' stride: in the row-major mode, where a
  // level's cap is its quota, the rounded-up slot count below is the larger of the two)
  plan->cand_total = std::max(cand_off, (out_cap + 15) & ~15);
  // slots per frame of the result blocks: the sum of the quotas, rounded up to 16 -- a describe workgroup's 16 slots
  // are then whole 64-byte lines of every section (fewer, full-line writes when the record goes to the host mirror)
  plan->out_cap = (out_cap + 15) & ~15;
  return ORBX_OK;
}

// entries of the resize-tap table of a plan (make_taps below fills them; at least one)
inline size_t taps_count(const OrbxPlan& plan) {
  size_t total = 0;
  for (int l = 1; l < plan.nlevels; l++) total += (size_t)align_up(plan.L[l].w, 4) + align_up(plan.L[l].h, 4);
  return total ? total : 1;
}

// 8-bit bilinear coefficient tables: OpenCV 4.x generic 8UC1 INTER_LINEAR path
// (imgproc/src/resize.cpp: scale = 1/((double)dst/src); fx = (float)((dx+0.5)*
// scale-0.5); sx = floor(fx); clamp with fx=0; 11-bit coefficients by cvRound).
// OpenCV is not part of this image: PARITY UNPINNED (DESIGN.md "Pyramid").
inline void make_taps(OrbxPlan& plan, std::vector<OrbxResizeTap>* taps) {
  taps->assign(taps_count(plan), OrbxResizeTap{0, 0, 0});
  for (int l = 1; l < plan.nlevels; l++) {
    const OrbxLevel& L = plan.L[l];
    const double scale_x = 1. / ((double)L.w / plan.w0), scale_y = 1. / ((double)L.h / plan.h0);
    for (int dx = 0; dx < L.w; dx++) {
      float fx = (float)((dx + 0.5) * scale_x - 0.5);
      int sx = (int)std::floor(fx);
      fx -= (float)sx;
      if (sx < 0) {
        fx = 0;
        sx = 0;
      }
      if (sx >= plan.w0 - 1) {
        fx = 0;
        sx = plan.w0 - 1;
      }
      OrbxResizeTap& t = (*taps)[L.xtab_off + dx];
      t.ofs = sx;
      t.c0 = (int16_t)std::lrintf((1.f - fx) * 2048.f);
      t.c1 = (int16_t)std::lrintf(fx * 2048.f);
      if (sx == plan.w0 - 1) {
        // src[w0-1]*c0 (+ src[w0-1]*0) == src[w0-2]*0 + src[w0-1]*c0: same sum, but the
        // kernel may now always fetch the pair (ofs, ofs+1) with one 16-bit load
        t.ofs = plan.w0 - 2;
        t.c1 = t.c0;
        t.c0 = 0;
      }
    }
    // can k_pyramid2 fetch the pairs of outputs 4g..4g+3 with one 8-byte window?
    {
      bool ok = plan.w0 >= 8;
      for (int dx = 0; dx + 3 < L.w && ok; dx += 4)
        ok = (*taps)[L.xtab_off + dx + 3].ofs + 1 - (*taps)[L.xtab_off + dx].ofs <= 7;
      // (a trailing partial group only adds padding taps with ofs 0, which the kernel never uses)
      for (int dx = L.w & ~3; dx < L.w && ok; dx++)
        ok = (*taps)[L.xtab_off + dx].ofs + 1 - (*taps)[L.xtab_off + (L.w & ~3)].ofs <= 7;
      plan.L[l].win8 = ok ? 1 : 0;
      if (!ok && plan.w0 >= 8) {
        // ... or stage the source rows of a strip through LDS (k_pyrblur): every 256-pixel strip of the level must
        // read its pairs from at most ORBX_PYR_STAGE_BYTES of a source row (scales up to ~3.2; orbx_internal.h).  The span starts at
        // the first pair, moved down so that its dwords END with the source row -- the buffer descriptor of the
        // frame returns zero for a dword that straddles the frame's last byte, which the dword holding the last
        // bytes of the last source row would do at any other alignment; where that is impossible (first strip: the
        // span cannot start before the row) the strip must not reach that dword.
        bool ok3 = true;
        for (int x0 = 0; x0 < L.w && ok3; x0 += ORBX_PYRBLUR_TW) {
          const int ofs_first = (*taps)[L.xtab_off + x0].ofs, ofs_last = (*taps)[L.xtab_off + std::min(x0 + 255, L.w - 1)].ofs;
          const int want = ofs_first - ((ofs_first - plan.w0) & 3), span0 = std::max(want, 0);
          ok3 = ofs_last + 2 - span0 <= ORBX_PYR_STAGE_BYTES;
          if (want < 0 && (plan.w0 & 3) && ofs_last + 2 > (plan.w0 & ~3)) ok3 = false;
        }
        if (ok3) plan.L[l].win8 = 3;
      }
    }
    for (int dy = 0; dy < L.h; dy++) {
      float fy = (float)((dy + 0.5) * scale_y - 0.5);
      int sy = (int)std::floor(fy);
      fy -= (float)sy;
      OrbxResizeTap& t = (*taps)[L.ytab_off + dy];
      t.ofs = sy;  // rows are clamped in the kernel, weights kept (OpenCV clips the row index only)
      t.c0 = (int16_t)std::lrintf((1.f - fy) * 2048.f);
      t.c1 = (int16_t)std::lrintf(fy * 2048.f);
    }
  }
}

// ---- what a context allocates for the tables of ANY frame it accepts ----------------------------------------------
// A context is created for max_width x max_height and takes every frame from 8 x 8 up to that size; each frame size
// gets its own tables (set_plan) in pools allocated once, from the plan of the maximum M.  Level sizes are monotone
// in the frame size (level_size: a rounded quotient by the same scale), and so is every table whose rows and columns
// are ceilings of a level's width / height over a constant -- all of them but the FAST table, whose tile rows are
// BALANCED and, with the adaptive first pass's preferred heights, clamped to "at most ORBX_MAX_BANDS / as many as
// the level above": neither is monotone in the height, so a frame a little smaller than the maximum can have more
// tile rows than the maximum itself has under any ONE preference vector.  Its capacity is therefore an upper bound
// that holds for every height up to the maximum's and every preference: per level, the maximum's units per tile row
// times the most tile rows make_bandmap can give a level of that height or less -- tile rows are never shorter than
// ORBX_MIN_TILE_H unless the level is, and never more than ORBX_MAX_BANDS in a table that make_bandmap accepts.
struct OrbxTableCapacity {
  size_t fast;   // FAST tile table (OrbxTileDesc entries per frame)
  size_t frame;  // blur, pyramid and fused pyramid + blur (whole / first pass / second pass) tables, each
  size_t small;  // fused pyramid + blur, short bands
  size_t taps;   // resize-tap table (OrbxResizeTap entries)
};
// Most strips the early bands add to a second-pass table of the fused pyramid + blur kernel (build_pyrblur_tiles with
// early_rows): a level's second pass then covers [P, S) and [S, h) in ceil((S - P) / RH) + ceil((h - S) / RH) bands
// with S - P <= ORBX_TOP_MARGIN <= RH, that is one band more than the ceil(h / RH) of the whole table at most,
// whatever h, the cut h0 and the depth D are.  (Strips per band grow with the width: the maximum's bound every size.)
static_assert(ORBX_TOP_MARGIN <= ORBX_PYRBLUR_RH, "an early band is one band");
inline size_t pyrblur_early_strips_bound(const OrbxPlan& M) {
  size_t n = 0;
  for (int l = 0; l < M.nlevels; l++) n += (size_t)pyrblur_strips_x(M.L[l].w);
  return n;
}
inline size_t fast_tiles_upper_bound(const OrbxPlan& M, int nms_radius, bool strips) {
  size_t cap = 0;
  for (int l = 0; l < M.nlevels; l++) {
    const int rows = std::min(ORBX_MAX_BANDS, (M.L[l].h + ORBX_MIN_TILE_H - 1) / ORBX_MIN_TILE_H);
    cap += (size_t)fast_tiles_x(M.L[l].w, nms_radius, strips) * (size_t)rows;
  }
  return cap;
}
// M: build_plan of the maximum (its win8 fields still zero: the pyramid tiles of the pool are then the short ones,
// ORBX_PYR2_TH rows -- the most: tests/cpp/plan_capacity_sweep.cpp compares with the real win8 of every frame).  Fails where the maximum itself has no FAST table (make_bandmap's reasons).
inline int table_capacity(const orbx_params& p, const OrbxPlan& M, int fast_impl, int blur_impl, OrbxTableCapacity* cap,
                          std::string* why) {
  OrbxBandMap bm;
  const int st = make_bandmap(M, p.nms_window / 2, &bm, why, fast_impl == 4, nullptr);
  if (st != ORBX_OK) return st;
  cap->fast = fast_tiles_upper_bound(M, p.nms_window / 2, fast_impl == 4);
  const size_t t1 = blur_tiles_for_impl(blur_impl, M, nullptr);
  const size_t t2 = build_frame_tiles(M, ORBX_PYR2_TW, ORBX_PYR2_TH, true, nullptr);
  const size_t t3 = build_pyrblur_tiles(M, ORBX_PYRBLUR_RH, nullptr);
  // (+ the extra bands of a split table, + the early bands of a second-pass table)
  cap->frame = std::max(std::max(t1, t2), t3) + 256 + pyrblur_early_strips_bound(M);
  cap->small = build_pyrblur_tiles(M, ORBX_PYRBLUR_RH_SMALL, nullptr) + 64;
  cap->taps = taps_count(M) + 16;
  return ORBX_OK;
}

// ---- where to cut the first pass of the FAST tile rows --------------------------------------------------------------
// The selection kernel counts, per level, the frames by the row in which their cap filled ("fill row" F = row of the
// cap-th survivor + 1; the level's height if it never filled) in buckets of ORBX_FILL_BUCKET_ROWS rows, the last
// bucket open-ended.  A unit of tile row 1 exits when the rows strictly above it hold `cap` survivors, that is for
// the frames with F <= rows of tile row 0.
#define ORBX_FILL_BUCKETS 32
#define ORBX_FILL_BUCKET_ROWS 4
inline int fill_bucket(int fill_row) { return std::min(std::max(fill_row - 1, 0) / ORBX_FILL_BUCKET_ROWS, ORBX_FILL_BUCKETS - 1); }
// feedback words of the top-rows-first pipeline (device, mirrored in pinned host memory by the batch's last kernel):
// [0] levels skipped, [1] levels produced (running totals), [2 + l] rows level l needed to fill its cap (maximum
// over the frames of the last batch; 0: not reported), [ORBX_FEEDBACK_HIST + l * ORBX_FILL_BUCKETS + b] frames of the
// last batch whose level l filled its cap in a row of bucket b (fill_bucket; the fused selection only)
#define ORBX_FEEDBACK_HIST (2 + ORBX_MAX_LEVELS)
#define ORBX_FEEDBACK_WORDS (ORBX_FEEDBACK_HIST + ORBX_MAX_LEVELS * ORBX_FILL_BUCKETS)
// frames known to have filled within the first `cut` rows: whole buckets only, so never a frame too many
inline uint32_t fill_exits(const uint32_t* hist, int cut) {
  uint32_t n = 0;
  for (int b = 0; b < ORBX_FILL_BUCKETS - 1 && ORBX_FILL_BUCKET_ROWS * (b + 1) <= cut; b++) n += hist[b];
  return n;
}
// What a unit of the streaming FAST kernel costs, in thousandths of a GROUP (7 centre rows: walk, candidate queue,
// segment test, NMS and mask store, ~570 instructions on the benchmark stream): a unit of `rows` rows walks
// ceil((rows + 2 R) / 7) groups after its set-up, and a unit that exits pays for its record and the probe.
// Counted in the kernel's assembly (tools/isa_stats.py --blocks, R = 1): the blocks before the group loop -- tile
// record, buffer descriptor, comparison table, clearing the score ring, the first 13 row loads, six rows into the
// LDS ring -- and the statistics after it are ~690 instructions; entry, record and probe of an exiting unit ~160.
#define ORBX_FAST4_UNIT_SETUP_MILLI 1200
#define ORBX_FAST4_UNIT_EXIT_MILLI 280
struct OrbxUnitCost {
  int setup_milli, exit_milli;
};
inline int fast4_unit_cost_milli(int rows, int nms_radius, const OrbxUnitCost& uc) {
  return uc.setup_milli + 1000 * ((rows + 2 * nms_radius + 6) / 7);
}
// expected cost of the first pass of one strip with tile row 0 of `cut` rows and tile row 1 of depth - cut
inline int first_pass_cost_milli(const uint32_t* hist, int depth, int cut, int nms_radius,
                                 const OrbxUnitCost& uc = OrbxUnitCost{ORBX_FAST4_UNIT_SETUP_MILLI, ORBX_FAST4_UNIT_EXIT_MILLI}) {
  uint64_t total = 0;
  for (int b = 0; b < ORBX_FILL_BUCKETS; b++) total += hist[b];
  const uint64_t out = total ? fill_exits(hist, cut) : 0, on = total ? total - out : 1;
  const uint64_t second = (on * (uint64_t)fast4_unit_cost_milli(depth - cut, nms_radius, uc) + out * (uint64_t)uc.exit_milli) /
                          (total ? total : 1);
  return fast4_unit_cost_milli(cut, nms_radius, uc) + (int)second;
}
// The rows of tile row 0 that make the first pass cheapest, among the cuts that end tile row 0 on a group boundary
// ((cut + 2 R) a multiple of 7) and leave both units within unit_max rows; 0: equal halves (an empty histogram, or
// no cut is cheaper than they are).  *cost_milli: the expected cost of what is returned.
inline int choose_first_cut(const uint32_t* hist, int depth, int nms_radius, int unit_max, int* cost_milli,
                            const OrbxUnitCost& uc = OrbxUnitCost{ORBX_FAST4_UNIT_SETUP_MILLI, ORBX_FAST4_UNIT_EXIT_MILLI}) {
  uint64_t total = 0;
  for (int b = 0; b < ORBX_FILL_BUCKETS; b++) total += hist[b];
  int best = 0, best_cost = first_pass_cost_milli(hist, depth, depth / 2, nms_radius, uc);
  if (total)
    for (int cut = 7 - (2 * nms_radius) % 7; cut < depth; cut += 7) {
      if (cut > unit_max || depth - cut > unit_max || cut == depth / 2) continue;
      // (a cut at which no frame exits only re-partitions the rows: whole groups are adapt_tile_rows' business)
      if (fill_exits(hist, cut) == 0) continue;
      const int c = first_pass_cost_milli(hist, depth, cut, nms_radius, uc);
      if (c < best_cost) {
        best = cut;
        best_cost = c;
      }
    }
  if (cost_milli) *cost_milli = best_cost;
  return best;
}

// ---- whether a level's early band pays (pyrblur_early_rows) ----------------------------------------------------------
// Per strip column, with q the share of frames that fill their cap within tile row 0 (fill row <= h0, from the same
// histogram): those frames save the band's rows and pay for a strip that leaves -- tile record, the probe of the
// tile-row statistic, return: ORBX_PYRBLUR_SKIP_EXIT instructions, counted in k_pyrblur's assembly along the path of a
// skipped strip that is not the reporter (profiles/pyramid_early_band) -- and the others pay the warm-up rows of one
// more band.  In the per-row instruction estimates of build_pyrblur_tiles:
//   q * rows * cost > (1 - q) * ORBX_PYRBLUR_WARMUP_ROWS * cost + q * ORBX_PYRBLUR_SKIP_EXIT
// Never for an empty histogram (nothing is known: 1080p, the LDS tile kernel), nor for a band of a row or two.
#define ORBX_PYRBLUR_SKIP_EXIT 100
#define ORBX_PYRBLUR_EARLY_MIN_ROWS 3
inline bool early_band_pays(const uint32_t* hist, int h0, int rows, int row_cost, int exit_cost = ORBX_PYRBLUR_SKIP_EXIT) {
  uint64_t total = 0;
  for (int b = 0; b < ORBX_FILL_BUCKETS; b++) total += hist[b];
  if (!total || rows < ORBX_PYRBLUR_EARLY_MIN_ROWS) return false;
  const uint64_t out = fill_exits(hist, h0), stay = total - out;
  return out * (uint64_t)rows * (uint64_t)row_cost >
         stay * (uint64_t)(ORBX_PYRBLUR_WARMUP_ROWS * row_cost) + out * (uint64_t)exit_cost;
}

}  // namespace orbx_geom
