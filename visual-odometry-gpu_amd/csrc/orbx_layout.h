// orbx_layout.h -- where the sections of every block of the host layer lie (result blocks, workspaces, scratch), and
// how many frames a workspace holds.  Host arithmetic on plain numbers, no HIP call: like orbx_plan.h it compiles
// into a stand-alone program (tests/cpp/layout_pins.cpp pins every value).  Not part of the public interface.
// A layout is a struct of byte offsets that its constructor computes from the block's shape: most take their sections
// from a private Sections base, member by member in the order of their declaration, which is the order in the block.
#pragma once
#include <algorithm>

#include "orbx_internal.h"

namespace orbx_layout {

using orbx_geom::align_up_sz;

// hands out the sections of a block one after another, each at a 256-byte boundary
struct Sections {
  size_t off = 0;  // where the next section starts: the block's size with its last section padded
  size_t end = 0;  // where the last section ends: the block's size without that padding
  size_t take(size_t bytes) {
    const size_t r = off;
    end = off + bytes;
    off = align_up_sz(end, 256);
    return r;
  }
};

// ---- the batched ORB path: the result block of n frames of cap slots ----
// sections: counts | kp16 | angle | desc || kp | lkp | resp | level -- what the reference's own output consists of
// (keypoints, orientations, descriptors: include/orb.hpp:37) first, so that orbx_batch_prefetch_compact moves one
// contiguous prefix of `compact` bytes (40 bytes per slot)
struct OutLayout : private Sections {
  size_t e, counts, kp16, angle, desc, compact, kp, lkp, resp, level, total;
  OutLayout() : OutLayout(0, 0) {}
  OutLayout(size_t n, size_t cap)
      : e(n * cap), counts(take(sizeof(int32_t) * n)), kp16(take(sizeof(uint32_t) * e)), angle(take(sizeof(float) * e)),
        desc(take(sizeof(orbx_descriptor) * e)), compact(off), kp(take(sizeof(orbx_keypoint) * e)),
        lkp(take(sizeof(orbx_keypoint) * e)), resp(take(sizeof(float) * e)), level(take(sizeof(int32_t) * e)),
        total(off) {}
};

// ---- Shi-Tomasi corners ----
// the workspace of m frames of w x h with a cell grid of grid_stride words per frame: response maps | key pools |
// cell grids | per-frame maxima, then candidate counts
struct GfLayout {
  size_t map, keys, grid, cnt, total, pool, grid_stride;
  GfLayout(int m, int w, int h, size_t grid_stride) : pool((size_t)(w - 2) * (h - 2)), grid_stride(grid_stride) {
    Sections s;
    map = s.take(sizeof(float) * (size_t)w * h * m);
    keys = s.take(sizeof(unsigned long long) * pool * m);
    grid = s.take(sizeof(uint32_t) * grid_stride * m);
    cnt = s.take(2 * sizeof(uint32_t) * (size_t)m);
    total = s.end;
  }
};
// the largest grid of a w x h frame: w * h cells of one slot (cell 1) or, from cell 2 on, at most
// ceil(w / 2) * ceil(h / 2) cells of four -- both within (w + 1)(h + 1) words
inline size_t gf_grid_bound(int w, int h) { return (size_t)(w + 1) * (h + 1); }
// the workspace of m frames of the largest size (+ 1024: the sections' alignment, whatever the frames' size)
inline size_t gf_workspace_bytes(int m, int max_w, int max_h) {
  return GfLayout(m, max_w, max_h, gf_grid_bound(max_w, max_h)).total + 1024;
}
// frames of the largest size that `limit` bytes hold: at least one, at most max_batch
inline size_t gf_workspace_frames(size_t limit, int max_w, int max_h, int max_batch) {
  return std::min<size_t>(std::max<size_t>(limit / gf_workspace_bytes(1, max_w, max_h), 1), (size_t)max_batch);
}
// frames of w x h per slice of n frames in a workspace of ws_bytes: what fits, in even slices
inline int gf_slice_frames(size_t ws_bytes, int n, int w, int h, size_t grid_stride) {
  const size_t one = GfLayout(1, w, h, grid_stride).total + 1024;  // (the sections' alignment: < 1024 bytes)
  const size_t fit = std::max<size_t>((ws_bytes - 1024) / one, 1);
  const int m = (int)std::min<size_t>(fit, (size_t)n);
  const int slices = (n + m - 1) / m;
  return (n + slices - 1) / slices;
}
// the result block: counts | corners
struct GrLayout : private Sections {
  size_t counts, corners, total;
  GrLayout(size_t n, size_t cap) : counts(take(sizeof(int32_t) * n)), corners(take(sizeof(float) * 2 * cap * n)), total(end) {}
};
// the bit maps of blocked pixels of m frames of w x h: the masked maxima first, then ceil(w / 32) * h words per frame
struct GbLayout : private Sections {
  size_t words, maxima, bits, total;
  GbLayout(size_t m, int w, int h)
      : words((size_t)((w + 31) / 32) * h), maxima(take(sizeof(uint32_t) * m)), bits(take(sizeof(uint32_t) * words * m)),
        total(end) {}
};
// the bit maps of m frames of the largest size (+ 512: whatever frames of a smaller size fit by gb_frames fit with
// their sections' alignment)
inline size_t gb_bytes(int m, int max_w, int max_h) { return GbLayout(m, max_w, max_h).total + 512; }
// frames of w x h whose bit maps and maxima fit bm_bytes (the maxima's alignment costs less than 256 bytes); at
// least one
inline size_t gb_frames(size_t bm_bytes, int w, int h) {
  return std::max<size_t>((bm_bytes - 256) / (sizeof(uint32_t) * (GbLayout(1, w, h).words + 1)), 1);
}
// the top-up's result block: counts | carried | points | origin
struct GtLayout : private Sections {
  size_t counts, carried, points, origin, total;
  GtLayout(size_t n, size_t cap)
      : counts(take(sizeof(int32_t) * n)), carried(take(sizeof(int32_t) * n)), points(take(sizeof(float) * 2 * cap * n)),
        origin(take(sizeof(int32_t) * cap * n)), total(end) {}
};

// ---- Lucas-Kanade ----
// buildOpticalFlowPyramid: halve ((w+1)/2) until a level would not be larger than the window
struct LkGeom {
  int top = 0;
  int w[ORBX_LK_MAX_LEVELS], h[ORBX_LK_MAX_LEVELS], pitch[ORBX_LK_MAX_LEVELS];
  size_t img_off[ORBX_LK_MAX_LEVELS], der_off[ORBX_LK_MAX_LEVELS];
  size_t img_bytes = 0, der_bytes = 0;
  LkGeom(int w0, int h0, int win, int max_level) {
    Sections img, der;
    for (int l = 0; l <= max_level; l++) {
      const int lw = l == 0 ? w0 : (w[l - 1] + 1) / 2, lh = l == 0 ? h0 : (h[l - 1] + 1) / 2;
      if (l > 0 && (lw <= win || lh <= win)) break;
      w[l] = lw;
      h[l] = lh;
      pitch[l] = lw;  // tight: a host image with stride == width goes up in ONE contiguous copy
      img_off[l] = img.take((size_t)pitch[l] * lh);
      der_off[l] = der.take((size_t)lw * lh * 4);
      top = l;
    }
    img_bytes = img.off;
    der_bytes = der.off;
  }
};
// the pair tracker's points, tight (they cross the bus whole, through one pinned mirror): prev | next | err | status
struct LkIo {
  size_t next, err, status, bytes;  // prev at 0
  explicit LkIo(size_t n) : next(sizeof(float) * 2 * n), err(2 * next), status(err + sizeof(float) * n), bytes(status + n) {}
};
// the windows tracker's workspace of ONE frame: the pyramid levels above 0 (level 0 is read in place), then the
// derivative maps of every level
struct LkwLayout {
  LkGeom g;
  size_t img_bytes, frame_bytes;  // levels 1 .. top; img_bytes + derivative maps
  LkwLayout(int w, int h, int win, int max_level) : g(w, h, win, max_level) {
    img_bytes = g.top >= 1 ? g.img_bytes - g.img_off[1] : 0;
    frame_bytes = img_bytes + g.der_bytes;
  }
};
// frames per slice: what `limit` bytes hold, at least one window, at most the batch
inline size_t lkw_fit(size_t limit, const LkwLayout& L, int window_len, int n_frames) {
  return std::min<size_t>(std::max<size_t>(limit / L.frame_bytes, (size_t)window_len), (size_t)n_frames);
}
// the workspace of a slice of m frames, [m][levels 1 .. top] | [m][levels 0 .. top] derivative maps: where the maps
// start, and its size
inline size_t lkw_der_offset(const LkwLayout& L, size_t m) { return align_up_sz(L.img_bytes * m, 256); }
inline size_t lkw_workspace_bytes(const LkwLayout& L, size_t m) { return m * L.frame_bytes + 256; }
// the windows tracker's result block: tracks | seen | err
struct LkwResult : private Sections {
  size_t slots, o_tracks, o_seen, o_err, bytes;
  LkwResult(size_t n_windows, size_t cap, size_t len)
      : slots(n_windows * cap), o_tracks(take(sizeof(float) * 2 * slots * len)), o_seen(take(sizeof(int32_t) * slots)),
        o_err(take(sizeof(float) * slots * (len - 1))), bytes(end) {}
};
// what the forward-backward check adds, in a buffer of its own: fb_d2 | lost
struct LkwFbResult : private Sections {
  size_t slots, o_d2, o_lost, bytes;
  LkwFbResult(size_t n_windows, size_t cap, size_t len)
      : slots(n_windows * cap), o_d2(take(sizeof(float) * slots * (len - 1))), o_lost(take(sizeof(int32_t) * slots)),
        bytes(end) {}
};

// ---- landmarks of n tracked windows of cap slots and len poses, and their bundle adjustment ----
// the result block: every array sized for every slot kept
struct LmBlock : private Sections {
  size_t slots, status, pose_off, pt_off, obs_off, slot, rows, points, oxy, opose, bytes;
  LmBlock(size_t n, size_t cap, size_t len)
      : slots(n * cap), status(take(sizeof(int32_t) * n)), pose_off(take(sizeof(int32_t) * (n + 1))),
        pt_off(take(sizeof(int32_t) * (n + 1))), obs_off(take(sizeof(int32_t) * (n + 1))),
        slot(take(sizeof(int32_t) * slots)), rows(take(sizeof(int32_t) * (slots + n))),
        points(take(sizeof(double) * 3 * slots)), oxy(take(sizeof(double) * 2 * slots * len)), opose(take(slots * len)),
        bytes(off) {}
};
// the scratch of a build
struct LmScratch : private Sections {
  size_t poses, gate, partial, keep, cand, bytes;
  LmScratch(size_t n, int cap, size_t len)
      : poses(take(sizeof(double) * 6 * n * len)), gate(take(sizeof(int32_t) * n)),
        partial(take(sizeof(int32_t) * 2 * n * orbx_lm_blocks(cap))), keep(take(n * cap)),
        cand(take(sizeof(double) * 3 * n * cap)), bytes(off) {}
};
// what the build from every view of a track (rank 15) adds, in a buffer of its own: the table of view records (16
// doubles per window and pose) | reason | reproj_px (one per slot)
struct LmViews : private Sections {
  size_t slots, table, reason, reproj_px, bytes;
  LmViews(size_t n, size_t cap, size_t len)
      : slots(n * cap), table(take(sizeof(double) * 16 * n * len)), reason(take(slots)),
        reproj_px(take(sizeof(float) * slots)), bytes(end) {}
};
// what a solve works on and leaves behind
struct LmSolve : private Sections {
  size_t poses, points, out, bytes;
  LmSolve(size_t n, size_t cap, size_t len)
      : poses(take(sizeof(double) * 6 * n * len)), points(take(sizeof(double) * 3 * n * cap)),
        out(take(sizeof(orbx_ba_summary) * n)), bytes(off) {}
};
// the workspaces of a solve's workgroups, for windows of at most cap landmarks and ocap observations: as many groups
// as windows, bounded by ORBX_BA_MAX_GROUPS and by the workspace budget.  Tracked windows of len poses: ocap = cap * len
struct LmWork {
  int groups;
  size_t wp, wo, slot, bytes;
  LmWork(int n, int cap, int len) : LmWork(n, (size_t)cap, (size_t)cap * len) {}
  LmWork(int n, size_t cap, size_t ocap) {
    Sections s;
    const size_t per_group = sizeof(double) * (ORBX_BA_WS_POINT * cap + ORBX_BA_WS_OBS * ocap) + 8 * cap;
    groups = std::min(n, ORBX_BA_MAX_GROUPS);
    groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, ORBX_BA_WS_BUDGET / per_group));
    wp = s.take(sizeof(double) * ORBX_BA_WS_POINT * cap * groups);
    wo = s.take(sizeof(double) * ORBX_BA_WS_OBS * ocap * groups);
    slot = s.take(8 * cap * groups);
    bytes = s.off;
  }
};
// the staged windows of orbx_bundle_adjust_batch, n windows with tp poses, tn landmarks and tm observations in all:
// the three offset tables (n + 1 entries each, back to back) | poses | points | rows | opose | oxy | summaries
struct BaStage : private Sections {
  size_t off, poses, points, rows, opose, oxy, out, bytes;
  BaStage(size_t n, size_t tp, size_t tn, size_t tm)
      : off(take(sizeof(int32_t) * 3 * (n + 1))), poses(take(sizeof(double) * 6 * tp)),
        points(take(sizeof(double) * 3 * tn)), rows(take(sizeof(int32_t) * (tn + n))), opose(take(tm)),
        oxy(take(sizeof(double) * 2 * tm)), out(take(sizeof(orbx_ba_summary) * n)), bytes(Sections::off) {}
};

// ---- pose and scale of tracked frame pairs ----
// the result block: one row of `cap` per pair in every per-position array
struct TpBlock : private Sections {
  size_t pairs, e, pose, n, scale, slot_of, mask, xyz, valid, bytes;
  TpBlock(size_t n_windows, size_t cap, size_t len)
      : pairs(n_windows * (len - 1)), e(pairs * cap), pose(take(sizeof(OrbxPoseOut) * pairs)),
        n(take(sizeof(int32_t) * pairs)), scale(take(sizeof(OrbxScaleOut) * pairs)), slot_of(take(sizeof(int32_t) * e)),
        mask(take(e)), xyz(take(sizeof(float) * 3 * e)), valid(take(e)), bytes(off) {}
};
// the scratch: the normalised point lists
inline size_t tp_scratch_bytes(int n_windows, int cap, int len) {
  return sizeof(OrbxPosePt) * (size_t)n_windows * (len - 1) * cap;
}

// ---- the poses of n tracked windows of len frames, chained on the device, and the write-back gate ----
// what goes up with a chain: T0 (16 doubles per window) | scale0 (one per window)
struct WpInput : private Sections {
  size_t T0, scale0, bytes;
  explicit WpInput(size_t n) : T0(take(sizeof(double) * 16 * n)), scale0(take(sizeof(double) * n)), bytes(end) {}
};
// the chain's result block: poses6 | poses4x4 | status
struct WpBlock : private Sections {
  size_t poses6, poses4x4, status, bytes;
  WpBlock(size_t n, size_t len)
      : poses6(take(sizeof(double) * 6 * n * len)), poses4x4(take(sizeof(double) * 16 * n * len)),
        status(take(sizeof(int32_t) * n)), bytes(off) {}
};
// the gate's result block: poses4x4 | updated (one byte per pose)
struct WbBlock : private Sections {
  size_t poses4x4, updated, bytes;
  WbBlock(size_t n, size_t len) : poses4x4(take(sizeof(double) * 16 * n * len)), updated(take(n * len)), bytes(off) {}
};

// ---- perspective-n-point over the landmarks block: n windows of len >= 3 frames of cap slots, one problem per
// (window, frame >= 2) ----
// the result block: records | seeded poses6 (n x len x 6) | mask (one row of cap bytes per problem)
struct PnpBlock : private Sections {
  size_t problems, records, poses6, mask, bytes;
  PnpBlock(size_t n, size_t cap, size_t len)
      : problems(n * (len - 2)), records(take(sizeof(OrbxPnpRecord) * problems)),
        poses6(take(sizeof(double) * 6 * n * len)), mask(take(problems * cap)), bytes(off) {}
};
// the scratch: every problem's gathered correspondences | the point each came from
struct PnpScratch : private Sections {
  size_t corr, cidx, bytes;
  PnpScratch(size_t n, size_t cap, size_t len)
      : corr(take(sizeof(OrbxPnpCorr) * n * (len - 2) * cap)), cidx(take(sizeof(int32_t) * n * (len - 2) * cap)),
        bytes(off) {}
};

// ---- landmarks carried into n windows of cap slots, and the PnP of every one of their len >= 2 frames against them ----
// the carry block: xyz (3 doubles per slot) | point (one per slot) | count (one per window)
struct CarryBlock : private Sections {
  size_t slots, xyz, point, count, bytes;
  CarryBlock(size_t n, size_t cap)
      : slots(n * cap), xyz(take(sizeof(double) * 3 * slots)), point(take(sizeof(int32_t) * slots)),
        count(take(sizeof(int32_t) * n)), bytes(off) {}
};
// the carried PnP's result block: records (one per (window, frame)) | poses6 (n x len x 6) | window_status (one per
// window) | mask (one row of cap bytes per problem)
struct CarryPnpBlock : private Sections {
  size_t problems, records, poses6, status, mask, bytes;
  CarryPnpBlock(size_t n, size_t cap, size_t len)
      : problems(n * len), records(take(sizeof(OrbxPnpRecord) * problems)), poses6(take(sizeof(double) * 6 * problems)),
        status(take(sizeof(int32_t) * n)), mask(take(problems * cap)), bytes(off) {}
};
// its scratch: every problem's gathered correspondences | the slot each came from | the problem's count
struct CarryPnpScratch : private Sections {
  size_t corr, cidx, ncorr, bytes;
  CarryPnpScratch(size_t n, size_t cap, size_t len)
      : corr(take(sizeof(OrbxPnpCorr) * n * len * cap)), cidx(take(sizeof(int32_t) * n * len * cap)),
        ncorr(take(sizeof(int32_t) * n * len)), bytes(off) {}
};
// what goes up with the one-window host entry: status (1) | pt_off (2) | slot_of_point | points3 (n_old each) | origin
// | seen (n_slots each) | tracks (n_slots x len x 2 floats)
struct CarryStage : private Sections {
  size_t status, pt_off, slot, points, origin, seen, tracks, bytes;
  CarryStage(size_t n_old, size_t n_slots, size_t len)
      : status(take(sizeof(int32_t))), pt_off(take(sizeof(int32_t) * 2)), slot(take(sizeof(int32_t) * n_old)),
        points(take(sizeof(double) * 3 * n_old)), origin(take(sizeof(int32_t) * n_slots)),
        seen(take(sizeof(int32_t) * n_slots)), tracks(take(sizeof(float) * 2 * n_slots * len)), bytes(off) {}
};

// ---- landmark priors of the landmarks block of n windows of cap slots (rank 20) ----
// the priors block: prior (anchor and weight, 4 doubles per landmark, in the block's point order) | count (one per
// window) | pt_off (a copy of the landmarks block's n + 1 point offsets: the priors stay fetchable after a rebuild)
struct PriorBlock : private Sections {
  size_t slots, prior, count, pt_off, bytes;
  PriorBlock(size_t n, size_t cap)
      : slots(n * cap), prior(take(sizeof(double) * 4 * slots)), count(take(sizeof(int32_t) * n)),
        pt_off(take(sizeof(int32_t) * (n + 1))), bytes(off) {}
};

// ---- descriptors at caller-held points of n frames of cap slots, and the re-association of two described sets ----
// the level-0 image of a w x h frame in the workspace: rows padded to a multiple of 4 bytes (describe_wave fetches
// aligned dwords), images a multiple of 256 bytes apart
inline int pd_pitch(int w) { return (w + 3) & ~3; }
inline size_t pd_img_stride(int w, int h) { return align_up_sz((size_t)pd_pitch(w) * h, 256); }
// frames of w x h per slice of n frames within `limit` bytes: what fits (at least one, at most a grid dimension's
// 65535), in even slices
inline int pd_slice_frames(size_t limit, int n, int w, int h) {
  const size_t fit = std::max<size_t>(limit / pd_img_stride(w, h), 1);
  const int m = (int)std::min<size_t>(std::min<size_t>(fit, (size_t)n), 65535);
  const int slices = (n + m - 1) / m;
  return (n + slices - 1) / slices;
}
// a bank's result block: desc (32 bytes per slot) | angle | state (one per slot each) | n_ok (one per frame)
struct PdBlock : private Sections {
  size_t slots, desc, angle, state, n_ok, bytes;
  PdBlock(size_t n, size_t cap)
      : slots(n * cap), desc(take(sizeof(orbx_descriptor) * slots)), angle(take(sizeof(float) * slots)),
        state(take(sizeof(int32_t) * slots)), n_ok(take(sizeof(int32_t) * n)), bytes(off) {}
};
// what goes up with the one-image host entry: the image (tight rows) | the points (two floats each)
struct PdStage : private Sections {
  size_t img, xy, bytes;
  PdStage(size_t w, size_t h, size_t n_points) : img(take(w * h)), xy(take(sizeof(float) * 2 * n_points)), bytes(off) {}
};
// the re-association's result block of n windows of qcap query slots: origin | dist (one per slot each) | count
struct RaBlock : private Sections {
  size_t slots, origin, dist, count, bytes;
  RaBlock(size_t n, size_t qcap)
      : slots(n * qcap), origin(take(sizeof(int32_t) * slots)), dist(take(sizeof(int32_t) * slots)),
        count(take(sizeof(int32_t) * n)), bytes(off) {}
};
// what goes up with the one-window host entry: query desc | query state | train desc | train state
struct RaStage : private Sections {
  size_t qdesc, qstate, tdesc, tstate, bytes;
  RaStage(size_t nq, size_t nt)
      : qdesc(take(sizeof(orbx_descriptor) * nq)), qstate(take(sizeof(int32_t) * nq)),
        tdesc(take(sizeof(orbx_descriptor) * nt)), tstate(take(sizeof(int32_t) * nt)), bytes(off) {}
};

// ---- the search by projection (rank 21) ----
// the projection's result block of n windows of cap old slots: xy (2 doubles per slot) | depth | state (one per slot
// each) | count (one per window)
struct SpBlock : private Sections {
  size_t slots, xy, depth, state, count, bytes;
  SpBlock(size_t n, size_t cap)
      : slots(n * cap), xy(take(sizeof(double) * 2 * slots)), depth(take(sizeof(double) * slots)),
        state(take(sizeof(int32_t) * slots)), count(take(sizeof(int32_t) * n)), bytes(off) {}
};
// what goes up with the one-window host entry: status (1) | pt_off (2) | slot_of_point | points3 (n_old each) | pose6
struct SpStage : private Sections {
  size_t status, pt_off, slot, points, pose6, bytes;
  explicit SpStage(size_t n_old)
      : status(take(sizeof(int32_t))), pt_off(take(sizeof(int32_t) * 2)), slot(take(sizeof(int32_t) * n_old)),
        points(take(sizeof(double) * 3 * n_old)), pose6(take(sizeof(double) * 6)), bytes(off) {}
};
// the gated re-association's scratch of n windows of tcap train slots: grids (one per window) | starts (cells_max + 1
// per window) | and the sorted list, one record per train slot: slot | xy (2 doubles) | desc (32 bytes)
struct SgScratch : private Sections {
  size_t slots, grids, starts, sslot, sxy, sdesc, bytes;
  SgScratch(size_t n, size_t tcap, size_t grid_bytes, size_t cells_max)
      : slots(n * tcap), grids(take(grid_bytes * n)), starts(take(sizeof(int32_t) * (cells_max + 1) * n)),
        sslot(take(sizeof(int32_t) * slots)), sxy(take(sizeof(double) * 2 * slots)), sdesc(take(32 * slots)),
        bytes(off) {}
};
// its block of its own beside the re-association's RaBlock: candidates (one per query slot)
struct SgBlock : private Sections {
  size_t slots, candidates, bytes;
  SgBlock(size_t n, size_t qcap) : slots(n * qcap), candidates(take(sizeof(int32_t) * slots)), bytes(off) {}
};
// what goes up with the one-window host entry: query desc | state | xy (2 floats) | train desc | state | xy (2 doubles)
// | pstate
struct SgStage : private Sections {
  size_t qdesc, qstate, qxy, tdesc, tstate, txy, tpstate, bytes;
  SgStage(size_t nq, size_t nt)
      : qdesc(take(32 * nq)), qstate(take(sizeof(int32_t) * nq)), qxy(take(sizeof(float) * 2 * nq)),
        tdesc(take(32 * nt)), tstate(take(sizeof(int32_t) * nt)), txy(take(sizeof(double) * 2 * nt)),
        tpstate(take(sizeof(int32_t) * nt)), bytes(off) {}
};

// ---- n overlapping windows of len frames, window w starting at stream frame w * stride, joined into one trajectory ----
// the frames of the stream
inline size_t st_stream_frames(size_t n, size_t len, size_t stride) { return (n - 1) * stride + len; }
// what goes up with a stitch and what its kernels hand one another: T_start (16 doubles) | links (14 doubles per
// window: R_rel, t_rel, b_first, b_link) | broken (one int32 per window)
struct StInput : private Sections {
  size_t T_start, links, broken, bytes;
  explicit StInput(size_t n)
      : T_start(take(sizeof(double) * 16)), links(take(sizeof(double) * 14 * n)), broken(take(sizeof(int32_t) * n)),
        bytes(end) {}
};
// the stitch's result block: trajectory4x4 | owner (one per stream frame) | anchors4x4 | lambda | status (one per window)
struct StBlock : private Sections {
  size_t frames, trajectory4x4, owner, anchors4x4, lambda, status, bytes;
  StBlock(size_t n, size_t len, size_t stride)
      : frames(st_stream_frames(n, len, stride)), trajectory4x4(take(sizeof(double) * 16 * frames)),
        owner(take(sizeof(int32_t) * frames)), anchors4x4(take(sizeof(double) * 16 * n)),
        lambda(take(sizeof(double) * n)), status(take(sizeof(int32_t) * n)), bytes(off) {}
};

// ---- the descriptor matcher, and pose and scale of the frame pairs of a batch ----
// one row of `cap` per pair in every per-slot array (e = pairs * cap slots).  The host-array entries use the same
// blocks with one pair: MatchBlock(1, nq), PoseBlock(1, max(n, 1)).
// the matcher's result block: idx | dist (two neighbours per slot) | match
struct MatchBlock : private Sections {
  size_t idx, dist, match, bytes;
  MatchBlock(size_t pairs, size_t cap)
      : idx(take(8 * pairs * cap)), dist(take(8 * pairs * cap)), match(take(4 * pairs * cap)), bytes(off) {}
};
// the staged input of the matcher's host entry: cnt (nq, nt) | q | t
struct MatchInput : private Sections {
  size_t cnt, q, t, bytes;
  MatchInput(size_t nq, size_t nt)
      : cnt(take(64)), q(take(sizeof(orbx_descriptor) * nq)),
        t(take(sizeof(orbx_descriptor) * std::max<size_t>(nt, 1))), bytes(off) {}
};
struct PoseBlock : private Sections {
  size_t pts, n, out, mask, bytes;
  PoseBlock(size_t pairs, size_t cap)
      : pts(take(sizeof(OrbxPosePt) * pairs * cap)), n(take(sizeof(int32_t) * pairs)),
        out(take(sizeof(OrbxPoseOut) * pairs)), mask(take(pairs * cap)), bytes(off) {}
};
// mq | mt: the compact match lists
struct ScaleBlock : private Sections {
  size_t xyz, valid, mq, mt, n, out, bytes;
  ScaleBlock(size_t pairs, size_t cap)
      : xyz(take(sizeof(float) * 3 * pairs * cap)), valid(take(pairs * cap)), mq(take(sizeof(int32_t) * pairs * cap)),
        mt(take(sizeof(int32_t) * pairs * cap)), n(take(sizeof(int32_t) * pairs)),
        out(take(sizeof(OrbxScaleOut) * pairs)), bytes(off) {}
};
// the two host-array entries of orbx_scale.hip lay out ONE buffer in turn.  orbx_triangulate of n points: in (both
// lists) | xyz | valid; orbx_estimate_scale of two lists of m points: prev, cur xyz | prev, cur valid | out
struct TriHost : private Sections {
  size_t in, xyz, valid, bytes;
  explicit TriHost(size_t n) : in(take(sizeof(float) * 4 * n)), xyz(take(sizeof(float) * 3 * n)), valid(take(n)), bytes(off) {}
};
struct ScaleHost : private Sections {
  size_t xyz, valid, out, bytes;
  explicit ScaleHost(size_t m)
      : xyz(take(sizeof(float) * 6 * m)), valid(take(2 * m)), out(take(sizeof(OrbxScaleOut))), bytes(off) {}
};

}  // namespace orbx_layout
