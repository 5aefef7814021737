// orbx_layout.h -- where the sections of every block of the host layer lie (result blocks, workspaces, scratch), and
// how many frames a workspace holds.  Host arithmetic on plain numbers, no HIP call: like orbx_plan.h it compiles
// into a stand-alone program (tests/cpp/layout_pins.cpp pins every value).  Not part of the public interface.
// A layout is a struct of byte offsets that its constructor computes from the block's shape.
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
struct OutLayout {
  size_t counts, kp16, kp, lkp, angle, resp, level, desc, compact, total;
  OutLayout() = default;
  OutLayout(int n, int cap) {
    Sections s;
    const size_t e = (size_t)n * (size_t)cap;
    counts = s.take(sizeof(int32_t) * (size_t)n);
    kp16 = s.take(sizeof(uint32_t) * e);
    angle = s.take(sizeof(float) * e);
    desc = s.take(sizeof(orbx_descriptor) * e);
    compact = s.off;
    kp = s.take(sizeof(orbx_keypoint) * e);
    lkp = s.take(sizeof(orbx_keypoint) * e);
    resp = s.take(sizeof(float) * e);
    level = s.take(sizeof(int32_t) * e);
    total = s.off;
  }
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
struct GrLayout {
  size_t corners, total;
  GrLayout(int n, int cap) {
    Sections s;
    s.take(sizeof(int32_t) * (size_t)n);
    corners = s.take(sizeof(float) * 2 * (size_t)cap * n);
    total = s.end;
  }
};
// the bit maps of blocked pixels of m frames of w x h: the masked maxima first, then ceil(w / 32) * h words per frame
struct GbLayout {
  size_t bits, words, total;
  GbLayout(int m, int w, int h) : words((size_t)((w + 31) / 32) * h) {
    Sections s;
    s.take(sizeof(uint32_t) * (size_t)m);
    bits = s.take(sizeof(uint32_t) * words * m);
    total = s.end;
  }
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
struct GtLayout {
  size_t carried, points, origin, total;
  GtLayout(int n, int cap) {
    Sections s;
    s.take(sizeof(int32_t) * (size_t)n);
    carried = s.take(sizeof(int32_t) * (size_t)n);
    points = s.take(sizeof(float) * 2 * (size_t)cap * n);
    origin = s.take(sizeof(int32_t) * (size_t)cap * n);
    total = s.end;
  }
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
struct LkwResult {
  size_t o_seen, o_err, bytes;  // tracks at 0
  LkwResult(int n_windows, int cap, int len) {
    Sections s;
    const size_t slots = (size_t)n_windows * cap;
    s.take(sizeof(float) * 2 * slots * len);
    o_seen = s.take(sizeof(int32_t) * slots);
    o_err = s.take(sizeof(float) * slots * (len - 1));
    bytes = s.end;
  }
};
// what the forward-backward check adds, in a buffer of its own: fb_d2 | lost
struct LkwFbResult {
  size_t o_lost, bytes;  // fb_d2 at 0
  LkwFbResult(int n_windows, int cap, int len) {
    Sections s;
    const size_t slots = (size_t)n_windows * cap;
    s.take(sizeof(float) * slots * (len - 1));
    o_lost = s.take(sizeof(int32_t) * slots);
    bytes = s.end;
  }
};

// ---- landmarks of n tracked windows of cap slots and len poses, and their bundle adjustment ----
// the result block: every array sized for every slot kept
struct LmBlock {
  size_t status, pose_off, pt_off, obs_off, slot, rows, points, oxy, opose, bytes;
  LmBlock(int n, int cap, int len) {
    Sections s;
    const size_t slots = (size_t)n * cap, noff = (size_t)n + 1;
    status = s.take(sizeof(int32_t) * n);
    pose_off = s.take(sizeof(int32_t) * noff);
    pt_off = s.take(sizeof(int32_t) * noff);
    obs_off = s.take(sizeof(int32_t) * noff);
    slot = s.take(sizeof(int32_t) * slots);
    rows = s.take(sizeof(int32_t) * (slots + n));
    points = s.take(sizeof(double) * 3 * slots);
    oxy = s.take(sizeof(double) * 2 * slots * len);
    opose = s.take(slots * len);
    bytes = s.off;
  }
};
// the scratch of a build
struct LmScratch {
  size_t poses, gate, partial, keep, cand, bytes;
  LmScratch(int n, int cap, int len) {
    Sections s;
    const size_t slots = (size_t)n * cap;
    poses = s.take(sizeof(double) * 6 * (size_t)n * len);
    gate = s.take(sizeof(int32_t) * n);
    partial = s.take(sizeof(int32_t) * 2 * (size_t)n * orbx_lm_blocks(cap));
    keep = s.take(slots);
    cand = s.take(sizeof(double) * 3 * slots);
    bytes = s.off;
  }
};
// what a solve works on and leaves behind
struct LmSolve {
  size_t poses, points, out, bytes;
  LmSolve(int n, int cap, int len) {
    Sections s;
    poses = s.take(sizeof(double) * 6 * (size_t)n * len);
    points = s.take(sizeof(double) * 3 * (size_t)n * cap);
    out = s.take(sizeof(orbx_ba_summary) * (size_t)n);
    bytes = s.off;
  }
};
// the workspaces of a solve's workgroups: as many groups as windows, bounded by ORBX_BA_MAX_GROUPS and by the
// workspace budget
struct LmWork {
  int groups;
  size_t wp, wo, slot, bytes;
  LmWork(int n, int cap, int len) {
    Sections s;
    const size_t ocap = (size_t)cap * len;
    const size_t per_group =
        sizeof(double) * ((size_t)ORBX_BA_WS_POINT * cap + (size_t)ORBX_BA_WS_OBS * ocap) + 8 * (size_t)cap;
    groups = std::min(n, ORBX_BA_MAX_GROUPS);
    groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, ORBX_BA_WS_BUDGET / per_group));
    wp = s.take(sizeof(double) * ORBX_BA_WS_POINT * (size_t)cap * groups);
    wo = s.take(sizeof(double) * ORBX_BA_WS_OBS * ocap * groups);
    slot = s.take(8 * (size_t)cap * groups);
    bytes = s.off;
  }
};

// ---- pose and scale of tracked frame pairs ----
// the result block: one row of `cap` per pair in every per-position array
struct TpBlock {
  size_t pose, n, scale, slot_of, mask, xyz, valid, bytes;
  TpBlock(int n_windows, int cap, int len) {
    Sections s;
    const size_t pairs = (size_t)n_windows * (len - 1), e = pairs * cap;
    pose = s.take(sizeof(OrbxPoseOut) * pairs);
    n = s.take(sizeof(int32_t) * pairs);
    scale = s.take(sizeof(OrbxScaleOut) * pairs);
    slot_of = s.take(sizeof(int32_t) * e);
    mask = s.take(e);
    xyz = s.take(sizeof(float) * 3 * e);
    valid = s.take(e);
    bytes = s.off;
  }
};
// the scratch: the normalised point lists
inline size_t tp_scratch_bytes(int n_windows, int cap, int len) {
  return sizeof(OrbxPosePt) * (size_t)n_windows * (len - 1) * cap;
}

}  // namespace orbx_layout
