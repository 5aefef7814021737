// layout_pins.cpp -- pins every block layout and every frames-per-slice value of csrc/orbx_layout.h to the formulas
// the host layer had before they were gathered there: each `want` below is the earlier code restated with its
// align_up_sz chain written out, and is compared with what the header gives over a sweep of shapes.  A mismatch prints
// the shape; the exit status is 1 if there was any.  Host only (tests/test_layouts.py compiles and runs it).
#include <cstdio>
#include <cstdlib>

#include "../../visual-odometry-gpu_amd/csrc/orbx_layout.h"

using namespace orbx_layout;

namespace {

long long g_checks = 0, g_failures = 0;
char g_shape[256];

void check(const char* what, size_t got, size_t want) {
  g_checks++;
  if (got == want) return;
  if (++g_failures <= 50) std::printf("FAIL %s: %s = %zu, want %zu\n", g_shape, what, got, want);
}
#define EQ(got, want) check(#got, (size_t)(got), (size_t)(want))
#define SHAPE(...) std::snprintf(g_shape, sizeof g_shape, __VA_ARGS__)

size_t A(size_t v) { return align_up_sz(v, 256); }

const int kN[] = {1, 2, 3, 7, 64, 256};
const int kSize[][2] = {{8, 8}, {9, 11}, {33, 8}, {320, 160}, {1241, 376}, {1920, 1080}};
const int kCap[] = {1, 16, 255, 256, 257, 2000};
const int kLen[] = {2, 3, 8};
const int kMinDistance[] = {0, 1, 2, 8};
const int kWin[] = {3, 21, 31};
const int kMaxLevel[] = {0, 3, 7};

// the cell grid's words per frame for a min_distance (gf_args of orbx_api_gftt.cpp)
size_t grid_stride(int w, int h, int min_distance) {
  if (min_distance < 1) return 0;
  const int cell = min_distance, gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
  return (size_t)gw * gh * (cell == 1 ? 1 : 4);
}

// ---- the earlier formulas ----
size_t old_gf_total(int m, int w, int h, size_t gs, size_t* keys, size_t* grid, size_t* cnt) {
  const size_t px = (size_t)w * h, pool = (size_t)(w - 2) * (h - 2);
  *keys = align_up_sz(sizeof(float) * px * m, 256);
  *grid = align_up_sz(*keys + sizeof(unsigned long long) * pool * m, 256);
  *cnt = align_up_sz(*grid + sizeof(uint32_t) * gs * m, 256);
  return *cnt + 2 * sizeof(uint32_t) * (size_t)m;
}
size_t old_gf_total(int m, int w, int h, size_t gs) {
  size_t a, b, c;
  return old_gf_total(m, w, h, gs, &a, &b, &c);
}
size_t old_gf_workspace_frames(size_t limit, int mw, int mh, int max_batch) {
  const size_t one = old_gf_total(1, mw, mh, (size_t)(mw + 1) * (mh + 1)) + 1024;
  return std::min<size_t>(std::max<size_t>(limit / one, 1), (size_t)max_batch);
}
int old_gf_slice_frames(size_t ws_bytes, int n, int w, int h, size_t gs) {
  const size_t one = old_gf_total(1, w, h, gs) + 1024;
  const size_t fit = std::max<size_t>((ws_bytes - 1024) / one, 1);
  const int m = (int)std::min<size_t>(fit, (size_t)n);
  const int slices = (n + m - 1) / m;
  return (n + slices - 1) / slices;
}
size_t old_gb_total(int m, int w, int h) {
  return align_up_sz(sizeof(uint32_t) * (size_t)m, 256) + sizeof(uint32_t) * ((size_t)((w + 31) / 32) * h) * m;
}
size_t old_gb_frames(size_t bm_bytes, int w, int h) {
  return std::max<size_t>((bm_bytes - 256) / (sizeof(uint32_t) * ((size_t)((w + 31) / 32) * h + 1)), 1);
}
// what a buffer of `bytes` asked for really holds (ensure / *_grow of the host layer)
size_t allocated(size_t bytes) { return align_up_sz(std::max<size_t>(bytes, 256), 256); }

void out_layout(int n, int cap) {
  SHAPE("out n=%d cap=%d", n, cap);
  const OutLayout o(n, cap);
  const size_t e = (size_t)n * (size_t)cap;
  size_t off = 0;
  EQ(o.counts, off), off = A(off + sizeof(int32_t) * (size_t)n);
  EQ(o.kp16, off), off = A(off + sizeof(uint32_t) * e);
  EQ(o.angle, off), off = A(off + sizeof(float) * e);
  EQ(o.desc, off), off = A(off + sizeof(orbx_descriptor) * e);
  EQ(o.compact, off);
  EQ(o.kp, off), off = A(off + sizeof(orbx_keypoint) * e);
  EQ(o.lkp, off), off = A(off + sizeof(orbx_keypoint) * e);
  EQ(o.resp, off), off = A(off + sizeof(float) * e);
  EQ(o.level, off), off = A(off + sizeof(int32_t) * e);
  EQ(o.total, off);
}

void good_features(int m, int w, int h, int min_distance) {
  const size_t gs = grid_stride(w, h, min_distance);
  SHAPE("gf m=%d %dx%d min_distance=%d", m, w, h, min_distance);
  const GfLayout o(m, w, h, gs);
  size_t keys, grid, cnt;
  const size_t total = old_gf_total(m, w, h, gs, &keys, &grid, &cnt);
  EQ(o.map, 0), EQ(o.keys, keys), EQ(o.grid, grid), EQ(o.cnt, cnt), EQ(o.total, total);
  EQ(o.pool, (size_t)(w - 2) * (h - 2)), EQ(o.grid_stride, gs);
  EQ(gf_grid_bound(w, h), (size_t)(w + 1) * (h + 1));
  const GbLayout b(m, w, h);
  EQ(b.words, (size_t)((w + 31) / 32) * h);
  EQ(b.bits, align_up_sz(sizeof(uint32_t) * (size_t)m, 256));
  EQ(b.total, old_gb_total(m, w, h));
}

// a context of max_w x max_h, max_batch frames and a workspace limit: the frames the workspace is made for, its size
// and the bit maps', and the frames per slice of every smaller frame size
void good_features_slices(int max_w, int max_h, int max_batch, size_t limit) {
  SHAPE("gf context %dx%d max_batch=%d limit=%zu", max_w, max_h, max_batch, limit);
  const size_t frames = gf_workspace_frames(limit, max_w, max_h, max_batch);
  EQ(frames, old_gf_workspace_frames(limit, max_w, max_h, max_batch));
  const size_t ws = gf_workspace_bytes((int)frames, max_w, max_h), bm = gb_bytes((int)frames, max_w, max_h);
  EQ(ws, old_gf_total((int)frames, max_w, max_h, (size_t)(max_w + 1) * (max_h + 1)) + 1024);
  EQ(bm, old_gb_total((int)frames, max_w, max_h) + 512);
  for (const auto& s : kSize) {
    if (s[0] > max_w || s[1] > max_h) continue;
    for (int n : kN) {
      if (n > max_batch) continue;
      for (int md : kMinDistance) {
        SHAPE("gf context %dx%d max_batch=%d limit=%zu: n=%d %dx%d min_distance=%d", max_w, max_h, max_batch, limit, n,
              s[0], s[1], md);
        const size_t gs = grid_stride(s[0], s[1], md);
        EQ(gf_slice_frames(allocated(ws), n, s[0], s[1], gs), old_gf_slice_frames(allocated(ws), n, s[0], s[1], gs));
      }
    }
    EQ(gb_frames(allocated(bm), s[0], s[1]), old_gb_frames(allocated(bm), s[0], s[1]));
  }
}

void good_features_results(int n, int cap) {
  SHAPE("gf results n=%d cap=%d", n, cap);
  const GrLayout r(n, cap);
  EQ(r.corners, align_up_sz(sizeof(int32_t) * (size_t)n, 256));
  EQ(r.total, align_up_sz(sizeof(int32_t) * (size_t)n, 256) + sizeof(float) * 2 * (size_t)cap * n);
  const GtLayout t(n, cap);
  const size_t carried = align_up_sz(sizeof(int32_t) * (size_t)n, 256);
  const size_t points = carried + align_up_sz(sizeof(int32_t) * (size_t)n, 256);
  const size_t origin = points + align_up_sz(sizeof(float) * 2 * (size_t)cap * n, 256);
  EQ(t.carried, carried), EQ(t.points, points), EQ(t.origin, origin);
  EQ(t.total, origin + sizeof(int32_t) * (size_t)cap * n);
}

void lucas_kanade(int w, int h, int win, int max_level) {
  SHAPE("lk %dx%d win=%d max_level=%d", w, h, win, max_level);
  const LkwLayout L(w, h, win, max_level);
  const LkGeom& g = L.g;
  int top = 0, lw[ORBX_LK_MAX_LEVELS], lh[ORBX_LK_MAX_LEVELS];
  size_t img_bytes = 0, der_bytes = 0;
  for (int l = 0; l <= max_level; l++) {
    const int cw = l == 0 ? w : (lw[l - 1] + 1) / 2, ch = l == 0 ? h : (lh[l - 1] + 1) / 2;
    if (l > 0 && (cw <= win || ch <= win)) break;
    lw[l] = cw, lh[l] = ch;
    EQ(g.w[l], cw), EQ(g.h[l], ch), EQ(g.pitch[l], cw);
    EQ(g.img_off[l], img_bytes), img_bytes += align_up_sz((size_t)cw * ch, 256);
    EQ(g.der_off[l], der_bytes), der_bytes += align_up_sz((size_t)cw * ch * 4, 256);
    top = l;
  }
  EQ(g.top, top), EQ(g.img_bytes, img_bytes), EQ(g.der_bytes, der_bytes);
  const size_t above0 = top >= 1 ? img_bytes - g.img_off[1] : 0, frame = above0 + der_bytes;
  EQ(L.img_bytes, above0), EQ(L.frame_bytes, frame);
  for (int len : kLen)
    for (int n_frames : {2, 3, 8, 64, 256}) {
      if (n_frames < len) continue;
      for (size_t limit : {(size_t)1, frame, 3 * frame + 1, (size_t)(7.5 * frame), (size_t)ORBX_LK_WORKSPACE_DEFAULT}) {
        SHAPE("lk %dx%d win=%d max_level=%d len=%d n_frames=%d limit=%zu", w, h, win, max_level, len, n_frames, limit);
        const size_t fit = std::min<size_t>(std::max<size_t>(limit / frame, (size_t)len), (size_t)n_frames);
        EQ(lkw_fit(limit, L, len, n_frames), fit);
        EQ(lkw_workspace_bytes(L, fit), fit * frame + 256);
        EQ(lkw_der_offset(L, fit), align_up_sz(above0 * fit, 256));
        EQ(lkw_der_offset(L, len), align_up_sz(above0 * len, 256));
      }
    }
}

void windows(int n, int cap, int len) {
  SHAPE("windows n=%d cap=%d len=%d", n, cap, len);
  const size_t slots = (size_t)n * cap, noff = (size_t)n + 1;
  {
    const LkwResult r(n, cap, len);
    const size_t o_seen = align_up_sz(sizeof(float) * 2 * slots * len, 256);
    const size_t o_err = align_up_sz(o_seen + sizeof(int32_t) * slots, 256);
    EQ(r.o_seen, o_seen), EQ(r.o_err, o_err), EQ(r.bytes, o_err + sizeof(float) * slots * (len - 1));
  }
  {
    const LmBlock b(n, cap, len);
    size_t off = 0;
    EQ(b.status, off), off = A(off + sizeof(int32_t) * n);
    EQ(b.pose_off, off), off = A(off + sizeof(int32_t) * noff);
    EQ(b.pt_off, off), off = A(off + sizeof(int32_t) * noff);
    EQ(b.obs_off, off), off = A(off + sizeof(int32_t) * noff);
    EQ(b.slot, off), off = A(off + sizeof(int32_t) * slots);
    EQ(b.rows, off), off = A(off + sizeof(int32_t) * (slots + n));
    EQ(b.points, off), off = A(off + sizeof(double) * 3 * slots);
    EQ(b.oxy, off), off = A(off + sizeof(double) * 2 * slots * len);
    EQ(b.opose, off), off = A(off + slots * len);
    EQ(b.bytes, off);
  }
  {
    const LmScratch s(n, cap, len);
    size_t off = 0;
    EQ(s.poses, off), off = A(off + sizeof(double) * 6 * (size_t)n * len);
    EQ(s.gate, off), off = A(off + sizeof(int32_t) * n);
    EQ(s.partial, off), off = A(off + sizeof(int32_t) * 2 * (size_t)n * ((cap + 255) / 256));
    EQ(s.keep, off), off = A(off + slots);
    EQ(s.cand, off), off = A(off + sizeof(double) * 3 * slots);
    EQ(s.bytes, off);
  }
  {
    const LmSolve v(n, cap, len);
    size_t off = 0;
    EQ(v.poses, off), off = A(off + sizeof(double) * 6 * (size_t)n * len);
    EQ(v.points, off), off = A(off + sizeof(double) * 3 * (size_t)n * cap);
    EQ(v.out, off), off = A(off + 32 * (size_t)n);  // orbx_ba_summary
    EQ(v.bytes, off);
  }
  {
    const LmWork w(n, cap, len);
    const int ocap = cap * len;
    const size_t per_group = sizeof(double) * ((size_t)30 * cap + (size_t)18 * ocap) + 8 * (size_t)cap;
    int groups = std::min(n, 512);
    groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, ((size_t)2 << 30) / per_group));
    size_t off = 0;
    EQ(w.groups, groups);
    EQ(w.wp, off), off = A(off + sizeof(double) * 30 * (size_t)cap * groups);
    EQ(w.wo, off), off = A(off + sizeof(double) * 18 * (size_t)ocap * groups);
    EQ(w.slot, off), off = A(off + 8 * (size_t)cap * groups);
    EQ(w.bytes, off);
  }
  {
    const TpBlock b(n, cap, len);
    const size_t pairs = (size_t)n * (len - 1), e = pairs * cap;
    size_t off = 0;
    EQ(b.pose, off), off = A(off + 184 * pairs);  // OrbxPoseOut
    EQ(b.n, off), off = A(off + sizeof(int32_t) * pairs);
    EQ(b.scale, off), off = A(off + 16 * pairs);  // OrbxScaleOut
    EQ(b.slot_of, off), off = A(off + sizeof(int32_t) * e);
    EQ(b.mask, off), off = A(off + e);
    EQ(b.xyz, off), off = A(off + sizeof(float) * 3 * e);
    EQ(b.valid, off), off = A(off + e);
    EQ(b.bytes, off);
    EQ(tp_scratch_bytes(n, cap, len), 32 * pairs * cap);  // OrbxPosePt
  }
}

// ---- matcher, pose, scale, bundle adjustment of staged windows, the pair tracker's points ----
// Before these parts held one block per call, every array below was a buffer of its own, asked of ensure() with the
// byte count written here and given that count rounded up to 256 (at least 256).  A block is that chain: every
// section where the sizes before it, each rounded up, end; at a multiple of 256; and at least as large as the request.
struct Chain {
  size_t off = 0;
  // a section the header puts at `got`, the next one (or the block's end) at `next`, for a buffer of `bytes`
  void sec(const char* what, size_t got, size_t next, size_t bytes) {
    check(what, got, off);
    check("offset % 256", got % 256, 0);
    check("section holds the request", next >= got && next - got >= bytes, 1);
    off = A(off + bytes);
  }
  void end(const char* what, size_t got) { check(what, got, off); }
};
#define SEC(ch, L, name, next, bytes) (ch).sec(#name, (L).name, (next), (bytes))

void match_block(int pairs, int cap) {
  const MatchBlock b(pairs, cap);
  const size_t e = (size_t)pairs * cap;
  Chain c;
  SEC(c, b, idx, b.dist, sizeof(int32_t) * 2 * e);
  SEC(c, b, dist, b.match, sizeof(int32_t) * 2 * e);
  SEC(c, b, match, b.bytes, sizeof(int32_t) * e);
  c.end("MatchBlock.bytes", b.bytes);
}
void pose_block(int pairs, int cap) {
  const PoseBlock b(pairs, cap);
  const size_t e = (size_t)pairs * cap;
  Chain c;
  SEC(c, b, pts, b.n, 32 * e);  // OrbxPosePt
  SEC(c, b, n, b.out, sizeof(int32_t) * (size_t)pairs);
  SEC(c, b, out, b.mask, 184 * (size_t)pairs);  // OrbxPoseOut
  SEC(c, b, mask, b.bytes, e);
  c.end("PoseBlock.bytes", b.bytes);
}
void scale_block(int pairs, int cap) {
  const ScaleBlock b(pairs, cap);
  const size_t e = (size_t)pairs * cap;
  Chain c;
  SEC(c, b, xyz, b.valid, sizeof(float) * 3 * e);
  SEC(c, b, valid, b.mq, e);
  SEC(c, b, mq, b.mt, sizeof(int32_t) * e);
  SEC(c, b, mt, b.n, sizeof(int32_t) * e);
  SEC(c, b, n, b.out, sizeof(int32_t) * (size_t)pairs);
  SEC(c, b, out, b.bytes, 16 * (size_t)pairs);  // OrbxScaleOut
  c.end("ScaleBlock.bytes", b.bytes);
}

// the host-array entries with n points (descriptors): the blocks of one pair, the staged inputs, the pair tracker
const int kHostN[] = {0, 1, 5, 255, 256, 257, 3000};
void host_entries(int n) {
  SHAPE("host entries n=%d", n);
  if (n > 0) {  // (every entry but orbx_estimate_pose returns before its buffers for n == 0)
    match_block(1, n);
    for (int nt : kHostN) {
      SHAPE("matcher input nq=%d nt=%d", n, nt);
      const MatchInput b(n, nt);
      Chain c;
      SEC(c, b, cnt, b.q, 64);
      SEC(c, b, q, b.t, 32 * (size_t)n);  // orbx_descriptor
      SEC(c, b, t, b.bytes, 32 * (size_t)std::max(nt, 1));
      c.end("MatchInput.bytes", b.bytes);
    }
    SHAPE("host entries n=%d", n);
    {
      const TriHost b(n);
      Chain c;
      SEC(c, b, in, b.xyz, sizeof(float) * 4 * (size_t)n);
      SEC(c, b, xyz, b.valid, sizeof(float) * 3 * (size_t)n);
      SEC(c, b, valid, b.bytes, (size_t)n);
      c.end("TriHost.bytes", b.bytes);
    }
    {
      const ScaleHost b(n);
      Chain c;
      SEC(c, b, xyz, b.valid, sizeof(float) * 6 * (size_t)n);
      SEC(c, b, valid, b.out, 2 * (size_t)n);
      SEC(c, b, out, b.bytes, 16);  // OrbxScaleOut
      c.end("ScaleHost.bytes", b.bytes);
    }
  }
  pose_block(1, n > 0 ? n : 1);
  // the pair tracker's points: tight, as orbx_lk_track had the offsets inline (one mirror, one copy each way)
  const LkIo io(n);
  const size_t o_out = sizeof(float) * 2 * (size_t)n, o_err = 2 * o_out, o_st = o_err + sizeof(float) * (size_t)n;
  EQ(io.next, o_out), EQ(io.err, o_err), EQ(io.status, o_st), EQ(io.bytes, o_st + (size_t)n);
}

// orbx_bundle_adjust_batch with n windows of W poses, N landmarks and M observations each
void ba_windows(int n, int W, int N, int M) {
  const size_t tp = (size_t)n * W, tn = (size_t)n * N, tm = (size_t)n * M;
  {
    const BaStage b(n, tp, tn, tm);
    Chain c;
    SEC(c, b, off, b.poses, sizeof(int32_t) * 3 * ((size_t)n + 1));
    SEC(c, b, poses, b.points, sizeof(double) * 6 * tp);
    SEC(c, b, points, b.rows, sizeof(double) * 3 * tn);
    SEC(c, b, rows, b.opose, sizeof(int32_t) * (tn + (size_t)n));
    SEC(c, b, opose, b.oxy, tm);
    SEC(c, b, oxy, b.out, sizeof(double) * 2 * tm);
    SEC(c, b, out, b.bytes, 32 * (size_t)n);  // orbx_ba_summary
    c.end("BaStage.bytes", b.bytes);
  }
  // the group count as orbx_bundle_adjust_batch had it, with cap = N and ocap = M
  const int cap = N, ocap = M;
  const size_t per_group = sizeof(double) * ((size_t)30 * cap + (size_t)18 * ocap) + 8 * (size_t)cap;
  int groups = std::min(n, 512);
  groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, ((size_t)2 << 30) / per_group));
  const LmWork w(n, (size_t)cap, (size_t)ocap);
  EQ(w.groups, groups);
  Chain c;
  SEC(c, w, wp, w.wo, sizeof(double) * 30 * (size_t)cap * groups);
  SEC(c, w, wo, w.slot, sizeof(double) * 18 * (size_t)ocap * groups);
  SEC(c, w, slot, w.bytes, 8 * (size_t)cap * groups);
  c.end("LmWork.bytes", w.bytes);
}

}  // namespace

int main() {
  static_assert(sizeof(OrbxPoseOut) == 184 && sizeof(OrbxScaleOut) == 16 && sizeof(OrbxPosePt) == 32 &&
                    sizeof(orbx_ba_summary) == 32,
                "the element types the layouts are made of");
  for (int n : kN)
    for (int cap : kCap) {
      out_layout(n, cap);
      good_features_results(n, cap);
      for (int len : kLen) windows(n, cap, len);
    }
  for (const auto& s : kSize) {
    for (int m : kN)
      for (int md : kMinDistance) good_features(m, s[0], s[1], md);
    for (int win : kWin)
      for (int max_level : kMaxLevel) lucas_kanade(s[0], s[1], win, max_level);
    // workspace limits from less than one frame's worth up to the default
    const size_t one = gf_workspace_bytes(1, s[0], s[1]);
    for (int max_batch : kN)
      for (size_t limit :
           {(size_t)1, one, 2 * one - 1, 3 * one, 7 * one + 5, 64 * one, (size_t)ORBX_GFTT_WORKSPACE_DEFAULT})
        good_features_slices(s[0], s[1], max_batch, limit);
  }
  for (int pairs = 1; pairs <= 256; pairs++)
    for (int cap = 1; cap <= 2000; cap++) {
      SHAPE("chain blocks pairs=%d cap=%d", pairs, cap);
      match_block(pairs, cap), pose_block(pairs, cap), scale_block(pairs, cap);
    }
  for (int n : kHostN) host_entries(n);
  for (int W = 2; W <= 8; W++)
    for (int N = 1; N <= 65536; N++)
      for (int n : {1, 5, 600})
        for (int M : {N, N * W}) {  // every landmark seen once, or by every pose
          SHAPE("ba n=%d W=%d N=%d M=%d", n, W, N, M);
          ba_windows(n, W, N, M);
        }
  std::printf("%lld values compared, %lld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
