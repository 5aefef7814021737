// orbx_api.cpp -- C-ABI host layer of liborbx.so (see include/orbx.h).
//
// Owns the context (device memory pools, stream, per-size plan), validates
// arguments, sequences the kernel launches of orbx_kernels.hip and moves
// results.  There is NO CPU fallback anywhere in this file: if the HIP
// runtime or a gfx950 device is missing every entry point fails loudly with
// ORBX_ERR_NO_DEVICE / ORBX_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "orbx_internal.h"
#include "orbx_tri_math.h"

using namespace orbx_geom;  // orbx_plan.h: the geometry of a frame size and the tables built from it

namespace {

thread_local std::string g_create_error;


struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// result block of a batch: one device allocation + one pinned host mirror so
// a whole batch comes back with a single D2H copy
// sections: counts | kp | angle | desc || lkp | resp | level -- what the reference's own output consists of
// (keypoints, orientations, descriptors: include/orb.hpp:37) first, so that orbx_batch_prefetch_compact moves one
// contiguous prefix of `compact` bytes
struct OutLayout {
  size_t counts, kp16, kp, lkp, angle, resp, level, desc, compact, total;
};

OutLayout make_out_layout(int n, int cap) {
  OutLayout o;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t r = off;
    off = align_up_sz(off + bytes, 256);
    return r;
  };
  const size_t e = (size_t)n * (size_t)cap;
  // the compact record first (orbx_batch_prefetch_compact copies [0, compact)): 40 bytes per slot
  o.counts = take(sizeof(int32_t) * (size_t)n);
  o.kp16 = take(sizeof(uint32_t) * e);
  o.angle = take(sizeof(float) * e);
  o.desc = take(sizeof(orbx_descriptor) * e);
  o.compact = off;
  o.kp = take(sizeof(orbx_keypoint) * e);
  o.lkp = take(sizeof(orbx_keypoint) * e);
  o.resp = take(sizeof(float) * e);
  o.level = take(sizeof(int32_t) * e);
  o.total = off;
  return o;
}

// One block of the ring of result blocks (orbx_ctx::blocks): the device allocation, its pinned host mirror and
// what the batch that last wrote it left there.
struct Block {
  uint8_t* d = nullptr;
  uint8_t* h = nullptr;      // pinned mirror
  uint8_t* h_dev = nullptr;  // the device-visible address of the pinned mirror
  OutLayout layout{};
  int n = 0;                  // frames in the block (0: never written)
  int cap = 1;                // slots per frame the block was written with
  bool copy_pending = false;  // an asynchronous D2H of the block has been enqueued (ev_copied)
  bool copy_compact = false;  // ... of its compact prefix only (orbx_batch_prefetch_compact)
  bool host_written = false;  // orbx_set_host_results: the describe kernel wrote the compact record to the mirror
  hipEvent_t ev_done = nullptr, ev_copied = nullptr;
  hipStream_t stream = nullptr;  // the stream of the batch that last wrote the block
};

// One lane of the pipelined mode: a set of working pools (pyramids, mask, statistics, candidates; sized for
// max_batch frames of max_width x max_height), the stream its batches run on, and the event / stream of the
// pools' last user.
struct Lane {
  uint8_t *d_pyr = nullptr, *d_pyr_blur = nullptr;
  unsigned long long *d_mask = nullptr, *d_row_stat = nullptr;
  orbx_keypoint* d_cand = nullptr;
  int32_t *d_cand_count = nullptr, *d_cand_total = nullptr;
  float* d_resp = nullptr;
  uint32_t* d_lcand = nullptr;  // spread selection: packed candidates, their responses, counts
  float* d_lresp = nullptr;
  int32_t* d_lcount = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_pool = nullptr;
  hipStream_t pool_stream = nullptr;
};

// a per-workgroup tile descriptor table (see OrbxTileDesc) of the current plan, in a pool sized for the largest frame
struct TileTable {
  OrbxTileDesc* d = nullptr;
  int count = 0;
  size_t capacity = 0;
};
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

// the events of one timed batched call
// (slots ORBX_NUM_STAGE_TIMES + 1, + 2: the boundaries inside the top-rows-first pipeline)
struct TimingSet {
  hipEvent_t ev[ORBX_NUM_STAGE_TIMES + 3] = {};
  int mode = 0;
  bool split = false;  // the call ran the top-rows-first pipeline
};

}  // namespace

// what a captured launch sequence depends on (run_batch)
struct OrbxGraphKey {
  const uint8_t* d_frames;
  size_t frame_stride;
  int n, w, h, row_stride, early, plan_serial, block;  // early: switches (early exit, fusion, two passes)
  bool operator==(const OrbxGraphKey& o) const {
    return d_frames == o.d_frames && frame_stride == o.frame_stride && n == o.n && w == o.w && h == o.h &&
           row_stride == o.row_stride && early == o.early && plan_serial == o.plan_serial && block == o.block;
  }
};

struct orbx_ctx {
  orbx_params p{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // geometry for the current frame size, and for the largest size (capacity)
  OrbxPlan plan{};
  OrbxPlan plan_max{};
  OrbxTileMap tm_blur{};  // 5x5 /273 variant (LDS tile kernel)
  OrbxBandMap bm_fast{};
  TileTable tiles[kTileTables];
  OrbxTopLevels top_levels{};  // the levels the second pass may skip
  DevBuf s_tiles;  // stage-API tables
  std::vector<OrbxResizeTap> h_taps;
  int plan_w = 0, plan_h = 0;

  uint8_t* d_in = nullptr;  // staged host frames, tight pitch (max_batch frames of max_width x max_height)
  // captured launch sequences of the most recent batch shapes (run_batch), round-robin replacement
  static constexpr int kGraphs = 16;  // (input, result block, lane) triples: 8 resident inputs over 4 blocks x 2 lanes
  hipGraphExec_t g_exec[kGraphs] = {};
  OrbxGraphKey g_key[kGraphs] = {};
  int g_next = 0;
  int plan_serial = 0;  // bumped whenever set_plan rebuilds the plan / tables
  OrbxResizeTap* d_taps = nullptr;
  size_t taps_capacity = 0;
  float* d_gauss = nullptr;
  // Result blocks.  A ring of kBlocks, used in turn by consecutive batches, each with a pinned host
  // mirror: the D2H copy of batch i (orbx_batch_prefetch, on its own copy stream) overlaps the
  // kernels of batch i+1, which write the other block.  blocks[blk] is the block of the most recent batch.
  // (a ring of kBlocks blocks: with two, the copy of batch i -- about as long as a step at 256 frames per batch --
  // had to finish before batch i + 2 could start; with four it overlaps two following batches)
  static constexpr int kBlocks = 4;
  Block blocks[kBlocks];
  int blk = 0;
  int host_results = 0;  // orbx_set_host_results: the describe kernel writes the compact record to the mirror
  int next_lane = 1;  // pipelined mode: the lane of the next batch (alternates)
  hipStream_t cstream = nullptr;
  // Pipelined batches (orbx_set_pipelined_batches): two LANES, each with its own stream and its own working pools;
  // consecutive device-resident batches alternate between them -- batch k uses lane k & 1 = its result block --
  // so the kernels of one batch overlap the tails and the nearly empty launches of the other.  lanes[0] has the
  // pools every context has, and its stream is the context's own; lanes[lane] is the lane of the most recent batch.
  // Stream order is the only ordering inside a lane.  A batch that comes to a lane's pools, or to a result block,
  // on ANOTHER stream than their previous user (a caller's stream, the other lane) first makes its stream wait for
  // that user's event: Lane::ev_pool / pool_stream for the pools of a lane, Block::ev_done / stream for a block.
  Lane lanes[2];
  int lane = 0;
  bool pipelined = false;
  bool last_two_pass = false;  // the last batch built its pyramid top rows first (enqueue_batch)
  hipStream_t last_stream = nullptr;

  // stage-API scratch (grown on demand; never touched by the batched path)
  DevBuf s_img_a, s_img_b, s_f32, s_u16, s_mask, s_kps, s_f32b, s_desc, s_i32, s_kern;
  DevBuf m_q, m_t, m_idx, m_dist, m_match, m_cnt;  // matcher (stage API and batch)
  // Lucas-Kanade tracker: two image pyramids (ping-pong: the `next` of one call is the
  // `prev` of the following one), the derivative pyramid of the current `prev`, point buffers
  DevBuf lk_img[2], lk_deriv, lk_io;  // lk_io: prev points | next points | err | status, one block
  void* lk_host = nullptr;            // pinned mirror of lk_io (one H2D + one D2H per call)
  size_t lk_host_bytes = 0;
  int lk_w = 0, lk_h = 0, lk_top = -1, lk_win = 0, lk_last = -1;  // lk_last: buffer holding the last `next`
  int match_pairs = 0;
  // batch serial: bumped by every batch run; match_serial: the serial the last batch match was made on
  long long batch_serial = 0, match_serial = -1;
  // bumped by every batch match: the pose step records the one it read (pose_match_gen), so the scale step, which
  // reads m_match again, can tell that the matches are still the ones the poses were computed from
  long long match_gen = 0, pose_match_gen = -1;
  // relative pose (orbx_pose.hip): batched results (pb_*) and the host-array entry's own buffers (ph_*)
  DevBuf pb_pts, pb_n, pb_out, pb_mask, ph_in, ph_pts, ph_n, ph_out, ph_mask;
  int pose_pairs = 0, pose_cap = 0;
  hipStream_t pose_stream = nullptr;
  long long pose_serial = -1;  // the batch serial the last batch pose ran on
  // triangulation and scale (orbx_scale.hip): batched results (sb_*: points, valid bytes, compact match lists,
  // match counts, scales) and the host-array entries' own buffers (sh_*)
  DevBuf sb_xyz, sb_valid, sb_mq, sb_mt, sb_n, sb_out, sh_in, sh_xyz, sh_valid, sh_out;
  int scale_pairs = 0, scale_cap = 0;
  hipStream_t scale_stream = nullptr;
  // bundle adjustment (orbx_ba.hip): the staged windows (offsets, parameter blocks, CSR observations), the
  // workgroups' workspaces and the summaries; grown on first use
  DevBuf ba_off, ba_poses, ba_points, ba_rows, ba_opose, ba_oxy, ba_wp, ba_wo, ba_slot, ba_out;
  // Shi-Tomasi corners (orbx_gftt.hip): the workspace of one slice of frames (response maps | key pools | cell grids
  // | per-frame maximum and candidate count), allocated on first use and bounded by gf_ws_limit; the staged host
  // image of the one-frame entries; and the entry's OWN result block (counts | corners), untouched by the ORB path
  DevBuf gf_ws, gf_img, gf_res;
  size_t gf_ws_limit = ORBX_GFTT_WORKSPACE_DEFAULT;
  int gf_n = 0, gf_cap = 0;  // frames and slots per frame of the last good-features batch (gf_n == 0: none)
  // the stream the last good-features call ran on, kept for COMPARISON only (a caller's stream may be gone by the
  // next call), and the event recorded behind that call's work: what later calls, fetches and orbx_destroy wait for
  hipStream_t gf_stream = nullptr;
  hipEvent_t gf_ev = nullptr;
  // Lucas-Kanade over frame windows (k_lk_track_windows): the workspace of one slice of frames (pyramid levels above
  // 0 | derivative maps), bounded by lkw_ws_limit; the window table; the staged frames and points of the one-window
  // host entry; and the entry's OWN result block (tracks | seen | err).  Nothing here is shared with orbx_lk_track.
  DevBuf lkw_ws, lkw_first, lkw_img, lkw_pts, lkw_res;
  size_t lkw_ws_limit = ORBX_LK_WORKSPACE_DEFAULT;
  int lkw_n = 0, lkw_cap = 0, lkw_len = 0;  // windows, slots per window, frames per window of the last call (0: none)
  hipStream_t lkw_stream = nullptr;  // for comparison only, as gf_stream
  hipEvent_t lkw_ev = nullptr;       // recorded behind every windows call
  void* lkw_first_host = nullptr;    // pinned mirror of the window table, and the event behind its upload
  size_t lkw_first_host_bytes = 0;
  hipEvent_t lkw_first_ev = nullptr;

  int timing = 0;  // 0 off, 1 all stages, 2 blur + fast only
  int fast_early = 1;
  int blur_impl = 2;  // ORBX_BLUR_IMPL, read at creation (launch_blur_auto)
  int fast_impl = 4;  // 4: streaming kernel (orbx_fast4.hip, the default), 3: LDS tile kernel (orbx_fast.hip); ORBX_FAST_IMPL, read at creation
  int fuse = 1;  // pyramid + blur in one kernel when blur runs on every level (orbx_set_fused_pyramid_blur)
  // Top-rows-first pipeline (enqueue_batch): 0 never, 1 whenever eligible, 2 adaptive -- the second pass
  // counts the (frame, level)s it skipped / had to produce (d_feedback, running totals, written to the pinned
  // h_feedback by the last kernel of every two-pass batch and read WITHOUT waiting at the start of later ones); while
  // fewer than a quarter are skipped the batches run in one pass, and every 128th one probes again.
  int top_mode = 2;
  bool top_on = true;          // the adaptive verdict
  int top_single_batches = 0;  // one-pass batches since the verdict turned negative
  uint32_t* d_feedback = nullptr;
  volatile uint32_t* h_feedback = nullptr;
  uint32_t feedback_seen[2] = {0, 0};
  // adaptive first pass (adapt_tile_rows): rows each level needed to fill its cap -- maximum of the current and of
  // the previous observation window --, the tile-row heights chosen from them (0: the default), bookkeeping
  uint32_t need_cur[ORBX_MAX_LEVELS] = {}, need_prev[ORBX_MAX_LEVELS] = {};
  int tile_h_pref[ORBX_MAX_LEVELS] = {};
  int need_batches = 0, need_window = 2, retiles = 0, learn_w = 0, learn_h = 0;
  bool prefs_applied = false;  // the current tile tables were built with tile_h_pref
  // ring of event sets: one per timed batched call, so that several calls can be
  // in flight before their stage times are read (no host sync between steps)
  TimingSet evr[ORBX_EVENT_SETS];
  long long ev_calls = 0;  // timed batched calls so far
  hipEvent_t ev[2] = {};   // orbx_bench_stage
};

namespace {

// Every entry point that takes a context runs on the context's device, whatever the caller's
// current device is (another context's, torch.cuda.set_device, ...), and leaves the caller's
// current device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(const orbx_ctx* c) {
    if (!c) return;
    enter(c->device);
  }
  explicit DeviceGuard(int dev) { enter(dev); }
  void enter(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int fail(orbx_ctx* c, int status, const std::string& msg) {
  if (c)
    c->err = msg;
  else
    g_create_error = msg;
  return status;
}

#define HIPCHK(c, expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return fail((c), ORBX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

int ensure(orbx_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return ORBX_OK;
  if (b.p) {  // nothing in flight may still use the old allocation: the context's stream, both lanes, a caller's stream
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const Lane& L : c->lanes)
      if (L.stream && L.stream != c->stream) HIPCHK(c, hipStreamSynchronize(L.stream));
    if (c->last_stream && c->last_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  bytes = align_up_sz(std::max<size_t>(bytes, 256), 256);
  HIPCHK(c, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return ORBX_OK;
}
#define ENSURE(c, buf, bytes)                        \
  do {                                               \
    const int _st = ensure((c), (buf), (bytes));     \
    if (_st != ORBX_OK) return _st;                  \
  } while (0)

// the stream the last batch ran on (the context's own before any batch)
hipStream_t batch_stream(const orbx_ctx* c) { return c->last_stream ? c->last_stream : c->stream; }
// the lane and the result block of the most recent batch
const Lane& cur_lane(const orbx_ctx* c) { return c->lanes[c->lane]; }
const Block& last_block(const orbx_ctx* c) { return c->blocks[c->blk]; }
// slots per frame of a result block written under plan P (nfeatures too small for any quota: one empty slot)
int slots_per_frame(const OrbxPlan& P) { return P.out_cap > 0 ? P.out_cap : 1; }

// an integer environment switch (the ones read once per process keep the value in a static of their reader)
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ORBX_PYR_GROUP=g: frames per dispatch group of the fused pyramid + blur kernel (0: frame-major grid)
int pyr_group_env() {
  static const int v = env_int("ORBX_PYR_GROUP", 32);
  return v;
}

// ORBX_TOP_ROWS=k: FAST tile rows of the first pass of the top-rows-first pipeline (0: one pass)
int top_rows_env() {
  static const int v = std::max(env_int("ORBX_TOP_ROWS", 2), 0);
  return v;
}

// Which FAST + NMS kernel the whole path runs: the register-streaming kernel (orbx_fast4.hip; the default) or, with
// ORBX_FAST_IMPL=3, the LDS tile kernel (orbx_fast.hip; always the stage operators').  Same results.  With every tile
// working they take the same time (+-2 %: 6.5 % fewer vector instructions against 14 instead of 24 waves per CU);
// in production -- the short tile rows of the adaptive first pass, most units exiting early -- the streaming kernel
// has less to do per unit (no tile fill, no barriers): same-box A/B 519 k vs 499 k frames/s (tools/ab_fast2.sh).
// Read when a context is created (A/B timing in one process).
int fast_impl_env() { return env_int("ORBX_FAST_IMPL", 4) == 3 ? 3 : 4; }

// 8-bit bilinear coefficient tables: OpenCV 4.x generic 8UC1 INTER_LINEAR path
// (imgproc/src/resize.cpp: scale = 1/((double)dst/src); fx = (float)((dx+0.5)*
// scale-0.5); sx = floor(fx); clamp with fx=0; 11-bit coefficients by cvRound).
// OpenCV is not part of this image: PARITY UNPINNED (DESIGN.md "Pyramid").
void make_taps(OrbxPlan& plan, std::vector<OrbxResizeTap>* taps) {
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

// createGaussianKernel (src/GaussianBlur.cpp:7-37), host side like the reference
int gaussian_kernel(int K, float sigma, float* kernel) {
  if (K <= 0 || (K % 2) == 0 || !kernel) return ORBX_ERR_INVALID_ARG;
  if (sigma <= 0.0f) sigma = 0.3f * ((K - 1) * 0.5f) + 0.8f;
  const int half = K / 2;
  float sum = 0.0f;
  for (int y = -half; y <= half; ++y)
    for (int x = -half; x <= half; ++x) {
      const float value = std::exp(-(float)(x * x + y * y) / (2 * sigma * sigma));
      kernel[(y + half) * K + (x + half)] = value;
      sum += value;
    }
  for (int i = 0; i < K * K; ++i) kernel[i] /= sum;
  return ORBX_OK;
}

int validate_params(const orbx_params& p, std::string* why) {
  auto bad = [&](const char* m) {
    *why = m;
    return (int)ORBX_ERR_INVALID_ARG;
  };
  if (p.nfeatures < 0) return bad("nfeatures < 0");
  if (!(p.scale_factor > 1.0f) || !(p.scale_factor <= 4.0f)) return bad("scale_factor must be in (1, 4]");
  if (p.nlevels < 1 || p.nlevels > ORBX_MAX_LEVELS) return bad("nlevels must be in [1, 16]");
  if (p.n < 1 || p.n > 16) return bad("n must be in [1, 16]");
  if (p.threshold < 0 || p.threshold > 255) return bad("threshold must be in [0, 255]");
  if (p.nms_window < 0 || p.nms_window / 2 > 3) return bad("nms_window must be in [0, 7]");
  if (p.patch_size < 1 || p.patch_size / 2 > 20) return bad("patch_size must be in [1, 41]");
  if (p.harris_window < 1 || (p.harris_window % 2) == 0 || p.harris_window > 15)
    return bad("harris_window must be odd, in [1, 15]");
  if (p.select_mode != ORBX_SELECT_HARRIS && p.select_mode != ORBX_SELECT_ROWMAJOR) return bad("select_mode");
  if (p.blur_levels < 0 || p.blur_levels > 2) return bad("blur_levels");
  if (p.blur_kind < 0 || p.blur_kind > 1) return bad("blur_kind");
  if (p.max_width < 8 || p.max_height < 8 || p.max_width > 16384 || p.max_height > 16384)
    return bad("max_width/max_height must be in [8, 16384]");
  if (p.max_batch < 1 || p.max_batch > 65535) return bad("max_batch must be in [1, 65535]");
  return ORBX_OK;
}

// The working pools of a lane, stated once: where the pointer lives, the bytes max_batch frames of the largest
// size need (0: no such pool in this context), and whether the pool starts out zeroed.
struct PoolRef {
  void** p;
  size_t bytes;
  bool zero;
};
std::array<PoolRef, 11> lane_pools(const orbx_ctx* c, Lane& L) {
  const OrbxPlan& M = c->plan_max;
  const size_t B = (size_t)c->p.max_batch, nc = B * (size_t)std::max(M.cand_total, 1);
  const size_t frames = B * (size_t)M.frame_bytes, levels = B * ORBX_MAX_LEVELS * sizeof(int32_t);
  return {{
      {(void**)&L.d_pyr, frames, false},
      // (zeroed: the padding bytes of a level stay zero, see set_plan; no pool when nothing is blurred)
      {(void**)&L.d_pyr_blur, c->p.blur_levels != ORBX_BLUR_NONE ? frames : 0, true},
      {(void**)&L.d_mask, B * (size_t)M.mask_words * 8, true},
      {(void**)&L.d_row_stat, B * ORBX_FAST_STAT_WORDS * 8, false},
      {(void**)&L.d_cand, nc * sizeof(orbx_keypoint), false},
      {(void**)&L.d_cand_count, levels, false},
      {(void**)&L.d_cand_total, levels, false},
      {(void**)&L.d_resp, nc * sizeof(float), false},
      {(void**)&L.d_lcand, nc * sizeof(uint32_t), false},
      {(void**)&L.d_lresp, nc * sizeof(float), false},
      {(void**)&L.d_lcount, levels, false},
  }};
}
hipError_t alloc_lane_pools(orbx_ctx* c, Lane& L) {
  for (const PoolRef& r : lane_pools(c, L)) {
    if (r.bytes == 0) continue;
    hipError_t e = hipMalloc(r.p, r.bytes + 256);  // (256 bytes of slack behind each pool)
    if (e == hipSuccess && r.zero) e = hipMemset(*r.p, 0, r.bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// the pools of a lane and the stream of the second one (nothing of the lane may be in flight)
void free_lane(orbx_ctx* c, Lane& L) {
  for (const PoolRef& r : lane_pools(c, L)) {
    if (*r.p) (void)hipFree(*r.p);
    *r.p = nullptr;
  }
  if (L.stream != c->stream) {  // (lane 0 runs on the context's own stream)
    if (L.stream) (void)hipStreamDestroy(L.stream);
    L.stream = nullptr;
  }
  L.pool_stream = nullptr;
}
// everything either lane has in flight has finished
hipError_t lanes_sync(orbx_ctx* c) {
  for (const Lane& L : c->lanes)
    if (L.stream) {
      const hipError_t e = hipStreamSynchronize(L.stream);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

bool fused_pyrblur(const orbx_ctx* c);
bool fast_early_on(const orbx_ctx* c);
int top_rows_env();
bool tile_prefs_apply(const orbx_ctx* c) {
  return c->top_mode == 2 && top_rows_env() > 0 && fast_early_on(c) && fused_pyrblur(c);
}

// a table of the new plan goes to its pool
int upload_tiles(orbx_ctx* c, int table, const std::vector<OrbxTileDesc>& t, const char* too_large) {
  TileTable& T = c->tiles[table];
  if (t.size() > T.capacity) return fail(c, ORBX_ERR_UNSUPPORTED, too_large);
  if (!t.empty())  // (no second pass / no FAST tile at all: nothing to copy)
    HIPCHK(c, hipMemcpy(T.d, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  T.count = (int)t.size();
  return ORBX_OK;
}

int set_plan(orbx_ctx* c, int w, int h) {
  if (w == c->plan_w && h == c->plan_h) return ORBX_OK;
  if (w < 8 || h < 8 || w > c->p.max_width || h > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame size outside [8, max_width] x [8, max_height]");
  OrbxPlan plan;
  std::string why;
  int st = build_plan(c->p, w, h, &plan, &why, c->fast_impl);
  if (st != ORBX_OK) return fail(c, st, why);
  make_taps(plan, &c->h_taps);
  if (c->h_taps.size() > c->taps_capacity) return fail(c, ORBX_ERR_UNSUPPORTED, "resize table exceeds pool");
  // the table may still be in use by an in-flight batch of the previous size
  HIPCHK(c, hipStreamSynchronize(batch_stream(c)));
  HIPCHK(c, lanes_sync(c));
  HIPCHK(c, hipMemcpy(c->d_taps, c->h_taps.data(), c->h_taps.size() * sizeof(OrbxResizeTap),
                      hipMemcpyHostToDevice));
  // no plan is set until every table below is in place: a call that fails on the way must not leave the previous
  // size's (plan_w, plan_h) standing for tables that are half replaced
  c->plan_w = c->plan_h = 0;
  c->plan = plan;
  // the fused pyramid + blur kernel writes only the dwords that hold image pixels; consumers rely on the
  // padding bytes of a level being zero (BRIEF's zero-extension), and another frame size re-uses the pool
  // (both lanes' pools; on the context's stream, and waited for: batches may run on a caller's stream)
  for (const Lane& L : c->lanes)
    if (L.d_pyr_blur)
      HIPCHK(c, hipMemsetAsync(L.d_pyr_blur, 0, (size_t)c->p.max_batch * (size_t)c->plan_max.frame_bytes, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  make_tilemap(plan, ORBX_BLUR_TW, ORBX_BLUR_TH, true, &c->tm_blur);
  // (the adaptive first pass's shorter tile rows only where the top-rows-first pipeline can run at all: with the
  // early exit or the fused kernel switched off every tile works, and the default rows have the smaller halo share)
  c->prefs_applied = tile_prefs_apply(c);
  st = make_bandmap(plan, c->p.nms_window / 2, &c->bm_fast, &why, c->fast_impl == 4,
                    c->prefs_applied ? c->tile_h_pref : nullptr);
  if (c->prefs_applied && (st != ORBX_OK || (size_t)c->bm_fast.band_begin[c->bm_fast.nbands] > c->tiles[T_FAST].capacity)) {
    // The learned tile rows give a table the pool cannot hold (the FAST table's capacity is an upper bound over every
    // preference, orbx_plan.h: this is a second line of defence).  What was learned is only a partition of the work:
    // forget it, take the default rows and run the batch -- a failure here would repeat with every batch of this size.
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) c->tile_h_pref[l] = 0;
    c->prefs_applied = false;
    st = make_bandmap(plan, c->p.nms_window / 2, &c->bm_fast, &why, c->fast_impl == 4, nullptr);
  }
  if (st != ORBX_OK) return fail(c, st, why);
  const bool grouped = pyr_group_env() > 0;
  const int top = top_rows_env();
  std::vector<OrbxTileDesc> t;
  blur_tiles_for_impl(c->blur_impl, plan, &t);
  if ((st = upload_tiles(c, T_BLUR, t, "blur tile table exceeds pool")) != ORBX_OK) return st;
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &t, grouped);
  if ((st = upload_tiles(c, T_PYRBLUR, t, "strip table exceeds pool")) != ORBX_OK) return st;
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &t, grouped, 1, &c->bm_fast, top);
  if ((st = upload_tiles(c, T_PYRBLUR_TOP, t, "strip table exceeds pool")) != ORBX_OK) return st;
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH, &t, grouped, 2, &c->bm_fast, top);
  if ((st = upload_tiles(c, T_PYRBLUR_REST, t, "strip table exceeds pool")) != ORBX_OK) return st;
  c->top_levels = OrbxTopLevels{};
  for (int l = 0; l < plan.nlevels; l++)
    if (pyrblur_first_pass_rows(plan, c->bm_fast, l, top) < plan.L[l].h) {
      const int i = c->top_levels.n++;
      c->top_levels.stat_index[i] = l * ORBX_MAX_BANDS;
      c->top_levels.rows[i] = std::min(top, c->bm_fast.tiles_y[l]);
      c->top_levels.cap[i] = plan.L[l].cap;
    }
  build_pyrblur_tiles(plan, ORBX_PYRBLUR_RH_SMALL, &t);
  if ((st = upload_tiles(c, T_PYRBLUR_SMALL, t, "strip table exceeds pool")) != ORBX_OK) return st;
  build_frame_tiles(plan, ORBX_PYR2_TW, ORBX_PYR2_TH, true, &t);
  if ((st = upload_tiles(c, T_PYR2, t, "pyramid tile table exceeds pool")) != ORBX_OK) return st;
  build_fast_tiles(plan, c->bm_fast, 0, 1, &t);
  if ((st = upload_tiles(c, T_FAST, t, "FAST tile table exceeds pool")) != ORBX_OK) return st;
  c->plan_serial++;
  c->plan_w = w;
  c->plan_h = h;
  return ORBX_OK;
}

hipError_t launch_pyramid_auto(orbx_ctx* c, hipStream_t s, int n, const uint8_t* d_in, int in_stride,
                               size_t in_frame_stride) {
  return orbx_launch_pyramid2(s, c->tiles[T_PYR2].d, c->tiles[T_PYR2].count, c->plan.frame_bytes, c->plan.w0, c->plan.h0, n,
                              d_in, in_stride, in_frame_stride, c->d_taps, cur_lane(c).d_pyr);
}


bool blur_enabled(const orbx_ctx* c) { return c->p.blur_levels != ORBX_BLUR_NONE; }
// ORBX_FUSE=0: separate pyramid and blur kernels (same results; A/B timing and per-kernel profiles)
bool fused_pyrblur(const orbx_ctx* c) {
  static const int env = env_int("ORBX_FUSE", 1);
  return env && c->fuse && c->p.blur_levels == ORBX_BLUR_ALL && c->p.blur_kind == ORBX_BLUR_SEP16;
}
const uint8_t* final_pyr(const orbx_ctx* c);

// FAST + NMS of the batched path.  Tiles that provably cannot contribute to the
// first `cap` row-major survivors exit early (see decode_band in the kernels);
// ORBX_FAST_EARLY=0 disables that (every tile does the full work).
int fast_early_env() {  // ORBX_FAST_EARLY=0: every tile does the full work (results are identical)
  static const int v = env_int("ORBX_FAST_EARLY", 1);
  return v;
}
bool fast_early_on(const orbx_ctx* c) { return fast_early_env() && c->fast_early; }

// FAST + NMS over tiles [first, first + count) of the context's band-major table
hipError_t launch_fast_tiles(orbx_ctx* c, hipStream_t s, int first, int count, int n, OrbxFastParams fp,
                             unsigned long long* stat, int chunk_scale = 1) {
  const OrbxTileDesc* tiles = c->tiles[T_FAST].d + first;
  unsigned long long* mask = cur_lane(c).d_mask;
  if (c->fast_impl == 4)
    return orbx_launch_fast4(s, tiles, count, n, final_pyr(c), c->plan.frame_bytes, c->plan.mask_words, fp, mask, stat);
  return orbx_launch_fast_nms(s, tiles, count, n, final_pyr(c), c->plan.frame_bytes, c->plan.mask_words, fp, mask, nullptr,
                              stat, chunk_scale);
}

hipError_t launch_fast_whole(orbx_ctx* c, hipStream_t s, int n, OrbxFastParams fp, bool stats_zeroed = false) {
  unsigned long long* stat = fast_early_on(c) ? cur_lane(c).d_row_stat : nullptr;
  if (stat && !stats_zeroed) {
    hipError_t e = hipMemsetAsync(stat, 0, (size_t)n * ORBX_FAST_STAT_WORDS * 8, s);
    if (e != hipSuccess) return e;
  }
  // (a two-launch variant -- tile row 0 first, the rest in strips of several tiles per
  // workgroup -- was measured slower: the kernel boundary costs more than the cheaper exits save)
  return launch_fast_tiles(c, s, 0, c->tiles[T_FAST].count, n, fp, stat);
}

// separable kind -> register-streaming kernel; /273 kind -> LDS tile kernel.
// ORBX_BLUR_IMPL (read when a context is created): 2 (default) k_blur3, 4 pixels per lane; 3: k_blur4, 16 pixels per
// lane (measured 9 % slower: the blur's vertical pass dominates its instruction count, and 94 registers leave 5
// waves per SIMD); 1: the first-generation LDS tile kernel.  The strip table is built for the kernel that reads it.
int blur_impl_env() {
  const int v = env_int("ORBX_BLUR_IMPL", 2);
  return v >= 1 && v <= 3 ? v : 2;
}
hipError_t launch_blur_auto(int impl, hipStream_t s, const OrbxPlan& P, const OrbxTileMap& tm1, const OrbxTileDesc* tiles2,
                            int ntiles2, int n, const uint8_t* src, uint8_t* dst, int first_level, int kind) {
  if (kind == ORBX_BLUR_SEP16 && impl == 3)
    return orbx_launch_blur4(s, tiles2, ntiles2, P.frame_bytes, n, src, dst, first_level);
  if (kind == ORBX_BLUR_SEP16 && impl != 1)
    return orbx_launch_blur3(s, tiles2, ntiles2, P.frame_bytes, n, src, dst, first_level);
  return orbx_launch_blur(s, P, tm1, n, src, dst, first_level, kind);
}
const uint8_t* final_pyr(const orbx_ctx* c) { return blur_enabled(c) ? cur_lane(c).d_pyr_blur : cur_lane(c).d_pyr; }

// Top-rows-first pipeline: wanted for the next batch?  (Eligibility -- fused kernel, early exit on, large
// batch -- is checked where the launches are made.)
bool top_rows_wanted(const orbx_ctx* c) {
  if (top_rows_env() <= 0 || c->top_mode == 0) return false;
  return c->top_mode == 1 || c->top_on;
}
// adaptive mode: look at the totals the second passes have reported so far (no waiting: whatever has arrived)
void top_rows_update(orbx_ctx* c) {
  if (c->top_mode != 2 || !c->h_feedback) return;
  // ONE 64-bit load of the pinned pair (the device writes it as one 8-byte store of two lanes' dwords at best: a torn
  // or stale pair, or a low half that has wrapped, only misleads this heuristic for one batch -- results never
  // depend on it)
  const uint64_t both = *reinterpret_cast<const volatile uint64_t*>(c->h_feedback);
  const uint32_t sk = (uint32_t)both, pr = (uint32_t)(both >> 32);
  const uint32_t dsk = sk - c->feedback_seen[0], dpr = pr - c->feedback_seen[1];
  if (dsk + dpr > 0) {
    c->feedback_seen[0] = sk;
    c->feedback_seen[1] = pr;
    const bool pays = 4ull * dsk >= (unsigned long long)(dsk + dpr);  // a quarter of the levels skipped
    if (!pays && c->top_on) c->top_single_batches = 0;
    c->top_on = pays;
  }
  if (!c->top_on && ++c->top_single_batches >= 128) {  // probe again
    c->top_on = true;
    c->top_single_batches = 0;
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
bool adapt_tile_rows(orbx_ctx* c) {
  if (!tile_prefs_apply(c) || !c->h_feedback || c->plan_w <= 0) return false;
  const int top = top_rows_env(), nl = c->plan.nlevels;
  bool any = false;
  for (int l = 0; l < nl; l++) {
    const uint32_t v = c->h_feedback[2 + l];  // (whatever has arrived; a stale or torn word only misleads the heuristic)
    if (v) {
      c->need_cur[l] = std::max(c->need_cur[l], std::min<uint32_t>(v, (uint32_t)c->plan.L[l].h));
      any = true;
    }
  }
  if (!any || ++c->need_batches < c->need_window) return false;
  // end of an observation window (2, 4, 8, 16, then every 32 batches)
  c->need_batches = 0;
  c->need_window = std::min(2 * c->need_window, 32);
  bool change = false, grow = false;
  int want[ORBX_MAX_LEVELS] = {};
  for (int l = 0; l < nl; l++) {
    const uint32_t need = std::max(c->need_cur[l], c->need_prev[l]);
    c->need_prev[l] = c->need_cur[l];
    c->need_cur[l] = 0;
    if (need == 0) {
      want[l] = c->tile_h_pref[l];
      continue;
    }
    const int rows = (int)need + std::max(4, (int)need / 10);  // margin: the next frames' caps may fill a little lower
    // the default tile rows of the level (make_bandmap: <= dflt rows, balanced)
    const int dflt = orbx_fast3_tile_h(c->p.nms_window / 2), lh = c->plan.L[l].h;
    const int bal = (lh + (lh + dflt - 1) / dflt - 1) / ((lh + dflt - 1) / dflt);
    int hh = (rows + top - 1) / top;
    // the streaming FAST kernel walks whole groups of 7 centre rows (tile rows + 2 x NMS radius): a height that is
    // one or two rows into a new group gives them back where at least 3 rows of margin remain (measured: level 0 at
    // 40 instead of 41 rows, FAST -4.6 %, pyramid -2.9 %; rounding every level to a group boundary costs more than
    // it saves)
    if (c->fast_impl == 4) {
      const int over = (hh + 2 * (c->p.nms_window / 2)) % 7;
      if ((over == 1 || over == 2) && top * (hh - over) >= (int)need + 3) hh -= over;
    }
    if (hh >= bal || lh <= top * hh) hh = 0;  // the default rows do
    const int eff = hh ? hh : bal, cur = c->bm_fast.tile_h[l], asked = c->tile_h_pref[l] ? c->tile_h_pref[l] : bal;
    // (a level that neither must grow nor gains three rows keeps its height when another level makes the tables change)
    want[l] = ((eff > cur && (int)need > top * cur) || eff + 2 < std::min(cur, asked)) ? hh : c->tile_h_pref[l];
    // the first pass has become too short for this stream -- caps fill BELOW it (the margin is used up): follow
    if (eff > cur && (int)need > top * cur) grow = true;
    // shrink only for a gain of three rows or more (`cur` may be taller than what was asked for: a level never has
    // more tile rows than the level above)
    else if (eff + 2 < std::min(cur, asked)) change = true;
  }
  if (!grow && !change) return false;
  if (!grow && c->retiles >= 4 && c->need_window < 32) return false;  // (settle first)
  for (int l = 0; l < nl; l++) c->tile_h_pref[l] = want[l];
  c->retiles++;
  return true;
}

// the launches of the whole path for n frames already on the device, into result block B (the plan, the current
// lane and the block's layout are set)
int enqueue_batch(orbx_ctx* c, Block& B, const uint8_t* d_frames, int n, int row_stride, size_t frame_stride, hipStream_t s) {
  const OrbxPlan& P = c->plan;
  const Lane& L = cur_lane(c);
  const TileTable &whole = c->tiles[T_PYRBLUR], &shortb = c->tiles[T_PYRBLUR_SMALL], &top = c->tiles[T_PYRBLUR_TOP],
                  &rest = c->tiles[T_PYRBLUR_REST];
  const int tm = c->timing;
  TimingSet& ts = c->evr[c->ev_calls % ORBX_EVENT_SETS];
  // event slots: 0 start | 1 pyramid | 2 blur | 3 fast | 4 compact | 5 harris | 6 select | 7 describe
  auto mark = [&](int slot, bool roofline_edge) -> hipError_t {
    if (tm == 1 || (tm == 2 && roofline_edge)) return hipEventRecord(ts.ev[slot], s);
    return hipSuccess;
  };
  const bool fused = fused_pyrblur(c);
  // (a wave per strip: below ~4096 waves the chip is far from full and the short-band table wins)
  const bool small = (long long)n * whole.count < 4096;
  // Top rows first.  The FAST early exit rests on the row-major cap (src/orb_cpu.cpp:108-110, src/orb.cpp:63):
  // once the top tile rows of a level hold `cap` survivors, nothing below them is ever looked at -- not by
  // FAST (its tiles exit), not by the selection (it stops at the first cap survivors), not by Harris or
  // the descriptors (their keypoints lie in those top rows).  So the pyramid is produced in two passes:
  //   1. the rows the first ORBX_TOP_ROWS FAST tile rows (and the descriptors of their keypoints) can read,
  //   2. FAST on those tile rows,
  //   3. the remaining rows -- a strip whose (frame, level) already has its cap survivors is skipped,
  //   4. FAST on the remaining tile rows (their tiles exit the same way).
  // What a skipped strip leaves in the pool (rows of an earlier batch) is never read.  Results are
  // identical either way (tests/test_gpu_parity.py, tests/test_batch64_parity.py).
  const bool two_pass = fused && !small && fast_early_on(c) && top_rows_wanted(c) && rest.count > 0 &&
                        c->bm_fast.nbands > top_rows_env();
  // tile-row statistics of the FAST early exit: zeroed up front so that the events around the FAST stage bracket
  // the kernel alone -- except in the top-rows-first pipeline, whose first pyramid pass clears them itself: a
  // memset node less per batch
  if (!two_pass) HIPCHK(c, hipMemsetAsync(L.d_row_stat, 0, (size_t)n * ORBX_FAST_STAT_WORDS * 8, s));
  HIPCHK(c, mark(0, false));
  OrbxFastParams fp{c->p.threshold, c->p.n, c->p.nms_window / 2};
  if (fused) {
    // blur on every level: pyramid and blur in one pass, the un-blurred pyramid is never materialised
    // (the event slots then read: pyramid = 0, blur = the fused kernel)
    HIPCHK(c, mark(1, true));
    if (!two_pass) {
      const TileTable& T = small ? shortb : whole;
      HIPCHK(c, orbx_launch_pyrblur(s, T.d, T.count, P.frame_bytes, P.w0, P.h0, n, d_frames, row_stride, frame_stride,
                                    c->d_taps, L.d_pyr_blur, small ? 0 : pyr_group_env()));
    } else {
      const int first_tiles = c->bm_fast.band_begin[top_rows_env()];
      HIPCHK(c, orbx_launch_pyrblur(s, top.d, top.count, P.frame_bytes, P.w0, P.h0, n, d_frames, row_stride, frame_stride,
                                    c->d_taps, L.d_pyr_blur, pyr_group_env(), nullptr, c->d_feedback, nullptr,
                                    L.d_row_stat));
      HIPCHK(c, mark(ORBX_NUM_STAGE_TIMES + 1, true));
      HIPCHK(c, launch_fast_tiles(c, s, 0, first_tiles, n, fp, L.d_row_stat));
      HIPCHK(c, mark(ORBX_NUM_STAGE_TIMES + 2, true));
      HIPCHK(c, orbx_launch_pyrblur(s, rest.d, rest.count, P.frame_bytes, P.w0, P.h0, n, d_frames, row_stride,
                                    frame_stride, c->d_taps, L.d_pyr_blur, pyr_group_env(), L.d_row_stat, c->d_feedback,
                                    &c->top_levels));
      HIPCHK(c, mark(2, true));
      HIPCHK(c, launch_fast_tiles(c, s, first_tiles, c->tiles[T_FAST].count - first_tiles, n, fp, L.d_row_stat, 4));
    }
  } else {
    HIPCHK(c, launch_pyramid_auto(c, s, n, d_frames, row_stride, frame_stride));
    HIPCHK(c, mark(1, true));
    if (blur_enabled(c))
      HIPCHK(c, launch_blur_auto(c->blur_impl, s, P, c->tm_blur, c->tiles[T_BLUR].d, c->tiles[T_BLUR].count, n, L.d_pyr,
                                 L.d_pyr_blur, c->p.blur_levels == ORBX_BLUR_UPPER ? 1 : 0, c->p.blur_kind));
  }
  if (!two_pass) {
    HIPCHK(c, mark(2, true));
    HIPCHK(c, launch_fast_whole(c, s, n, fp, true));
  }
  ts.split = two_pass;
  c->last_two_pass = two_pass;
  HIPCHK(c, mark(3, true));
  HIPCHK(c, mark(4, false));  // (compaction, Harris and selection are one kernel: its time is the "select" slot)
  HIPCHK(c, mark(5, false));
  const OutLayout& o = B.layout;
  // ORBX_SELECT_SPREAD=0/1 forces the fused / the three-kernel selection (A/B timing); frames whose candidates do not
  // fit the fused kernel's LDS take the three kernels whatever it says (orbx_launch_level_select_auto)
  static const int spread = env_int("ORBX_SELECT_SPREAD", -1);
  HIPCHK(c, orbx_launch_level_select_auto(s, P, n, c->p.select_mode, spread, L.d_mask, final_pyr(c), c->d_gauss,
                                          c->p.harris_window, c->p.harris_k, L.d_lcand, L.d_lcount, L.d_lresp,
                                          L.d_cand, L.d_resp, L.d_cand_count, two_pass ? c->d_feedback + 2 : nullptr));
  HIPCHK(c, mark(6, false));
  if (P.out_cap <= 0)  // nfeatures too small for any quota: no describe launch, so the counts are zeroed here
    HIPCHK(c, hipMemsetAsync(B.d + o.counts, 0, sizeof(int32_t) * (size_t)n, s));
  // orbx_set_host_results: the kernel also writes the compact record into the pinned mirror of the block
  OrbxHostRecord hr{};
  if (c->host_results && P.out_cap > 0 && B.h_dev)
    hr = OrbxHostRecord{(int32_t*)(B.h_dev + o.counts), (uint32_t*)(B.h_dev + o.kp16), (float*)(B.h_dev + o.angle),
                        (orbx_descriptor*)(B.h_dev + o.desc)};
  HIPCHK(c, orbx_launch_describe(s, P, n, final_pyr(c), c->p.patch_size, L.d_cand_count, L.d_cand, L.d_resp,
                                 (int32_t*)(B.d + o.counts), (orbx_keypoint*)(B.d + o.lkp),
                                 (float*)(B.d + o.resp), (int32_t*)(B.d + o.level),
                                 (orbx_keypoint*)(B.d + o.kp), (uint32_t*)(B.d + o.kp16),
                                 (float*)(B.d + o.angle),
                                 (orbx_descriptor*)(B.d + o.desc), two_pass ? c->d_feedback : nullptr,
                                 two_pass ? const_cast<uint32_t*>(c->h_feedback) : nullptr, &hr));
  HIPCHK(c, mark(7, false));
  return ORBX_OK;
}

// The launch sequence of a batch depends only on (input pointer and strides, n, plan, switches): it
// is captured once into a hipGraph and replayed with one hipGraphLaunch per batch (7 enqueues ->
// 1; matters most for the one-frame-per-call shape, which is launch-bound).  Stage timing needs
// event records between the kernels, so it takes the plain path.  ORBX_GRAPH=0 disables.
void drop_graph(orbx_ctx* c, int i) {
  if (c->g_exec[i]) (void)hipGraphExecDestroy(c->g_exec[i]);
  c->g_exec[i] = nullptr;
}

int run_batch(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
              hipStream_t s, bool may_pipeline = false) {
  // Pipelined mode: a device-resident batch on the context's stream goes to the lane of its result block -- own
  // pools, own stream, so nothing of the other lane's batch in flight is touched.  (The plan's tables are shared:
  // set_plan waits for both lanes before it changes them.)
  // adaptive first pass (adapt_tile_rows): what was learned belongs to one frame size; new tile-row heights make
  // set_plan below rebuild the tables (it waits for the batches in flight; this batch then runs unpipelined)
  if (w != c->learn_w || h != c->learn_h) {
    c->learn_w = w;
    c->learn_h = h;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) c->need_cur[l] = c->need_prev[l] = 0, c->tile_h_pref[l] = 0;
    for (int i = 2; i < ORBX_FEEDBACK_WORDS; i++) c->h_feedback[i] = 0;
    c->need_batches = 0;
    c->need_window = 2;
    c->retiles = 0;
  } else if (w == c->plan_w && h == c->plan_h) {
    bool any_pref = false;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) any_pref |= c->tile_h_pref[l] != 0;
    // (a switch that takes the top-rows-first pipeline away, or brings it back, since the tables were built)
    if (adapt_tile_rows(c) || (any_pref && tile_prefs_apply(c) != c->prefs_applied)) c->plan_w = 0;
  }
  const bool lanes = may_pipeline && c->pipelined && s == c->stream && w == c->plan_w && h == c->plan_h;
  c->lane = lanes ? c->next_lane : 0;
  Lane& L = c->lanes[c->lane];
  if (lanes) {
    s = L.stream;
  } else {
    if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
    // the pools (pyramids, mask, result block) are reused by every batch: a batch still in
    // flight on a DIFFERENT stream must have finished before this one may touch them
    if (c->last_stream && c->last_stream != s) HIPCHK(c, hipStreamSynchronize(c->last_stream));
  }
  int st = set_plan(c, w, h);
  if (st != ORBX_OK) return st;
  top_rows_update(c);
  // this batch writes the other result block; if that block is still the source of an
  // asynchronous D2H copy (orbx_batch_prefetch two batches ago), the kernels wait for the copy
  const int blk = (c->blk + 1) % orbx_ctx::kBlocks;
  Block& B = c->blocks[blk];
  if (B.copy_pending) HIPCHK(c, hipStreamWaitEvent(s, B.ev_copied, 0));
  // the previous users of this lane's pools and of this result block, if they ran on another stream (a batch on a
  // caller's stream between pipelined batches, or the other way round): device-side waits, no host stall
  if (L.pool_stream && L.pool_stream != s) HIPCHK(c, hipStreamWaitEvent(s, L.ev_pool, 0));
  if (B.stream && B.stream != s) HIPCHK(c, hipStreamWaitEvent(s, B.ev_done, 0));
  // The block becomes "the last batch" only once its launches are enqueued (B.n and c->blk below): after a failed
  // call orbx_batch_fetch must not hand out what an older batch left in it.
  B.n = 0;
  B.copy_pending = false;
  B.copy_compact = false;
  // result block sections are laid out for (n, pool slot capacity)
  B.cap = slots_per_frame(c->plan);
  B.layout = make_out_layout(n, B.cap);
  static const int use_graph = env_int("ORBX_GRAPH", 1);
  const int tm = c->timing;
  if (use_graph && tm == 0) {
    const OrbxGraphKey key{d_frames, frame_stride, n, w, h, row_stride, (fast_early_on(c) ? 1 : 0) | (fused_pyrblur(c) ? 2 : 0) | (top_rows_wanted(c) ? 4 : 0) | (lanes ? 8 : 0) | (c->lane << 4) | (c->host_results ? 64 : 0),
                           c->plan_serial, blk};
    int gi = -1;
    for (int i = 0; i < orbx_ctx::kGraphs; i++)
      if (c->g_exec[i] && key == c->g_key[i]) gi = i;
    if (gi < 0) {
      gi = c->g_next;
      c->g_next = (c->g_next + 1) % orbx_ctx::kGraphs;
      drop_graph(c, gi);
      hipGraph_t g = nullptr;
      const hipError_t be = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
      if (be != hipSuccess) return fail(c, ORBX_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(be));
      st = enqueue_batch(c, B, d_frames, n, row_stride, frame_stride, s);
      const hipError_t ee = hipStreamEndCapture(s, &g);
      if (st != ORBX_OK) {
        if (g) (void)hipGraphDestroy(g);
        return st;
      }
      if (ee != hipSuccess) return fail(c, ORBX_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
      const hipError_t ie = hipGraphInstantiate(&c->g_exec[gi], g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (ie != hipSuccess) {
        c->g_exec[gi] = nullptr;
        return fail(c, ORBX_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
      }
      c->g_key[gi] = key;
    }
    const hipError_t le = hipGraphLaunch(c->g_exec[gi], s);
    if (le != hipSuccess) return fail(c, ORBX_ERR_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(le));
  } else {
    if ((st = enqueue_batch(c, B, d_frames, n, row_stride, frame_stride, s)) != ORBX_OK) return st;
  }
  c->blk = blk;
  if (lanes) c->next_lane ^= 1;
  c->batch_serial++;
  c->last_stream = s;
  B.n = n;
  B.host_written = c->host_results && c->plan.out_cap > 0;
  HIPCHK(c, hipEventRecord(B.ev_done, s));
  if (B.host_written) {
    // orbx_set_host_results: the compact record is in the pinned mirror when the batch ends -- the block counts as
    // compact-copied from the start (the copy stream is not involved; orbx_batch_prefetch_compact has nothing to do)
    HIPCHK(c, hipEventRecord(B.ev_copied, s));
    B.copy_pending = true;
    B.copy_compact = true;
  }
  HIPCHK(c, hipEventRecord(L.ev_pool, s));
  L.pool_stream = s;
  B.stream = s;
  if (tm != 0) {
    c->evr[c->ev_calls % ORBX_EVENT_SETS].mode = tm;
    c->ev_calls++;
  }
  return ORBX_OK;
}

int check_image(orbx_ctx* c, const void* img, int w, int h, int stride) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!img) return fail(c, ORBX_ERR_INVALID_ARG, "image is NULL");
  if (w < 8 || h < 8 || w > c->p.max_width || h > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "image size outside [8, max_width] x [8, max_height]");
  if (stride < w) return fail(c, ORBX_ERR_INVALID_ARG, "stride < width");
  return ORBX_OK;
}

// single-level plan over a scratch image, for the stage-level operators
OrbxPlan flat_plan(int w, int h, int cap) {
  OrbxPlan P;
  std::memset(&P, 0, sizeof(P));
  P.nlevels = 1;
  P.w0 = w;
  P.h0 = h;
  OrbxLevel& L = P.L[0];
  L.w = w;
  L.h = h;
  L.pitch = align_up(w, 64);
  L.mask_wpr = (w + 63) / 64;
  L.cap = cap;
  L.quota = cap;
  L.scale = 1.0f;
  P.frame_bytes = (int32_t)align_up_sz((size_t)L.pitch * h, 256);
  P.mask_words = L.mask_wpr * h;
  P.cand_total = cap;
  P.out_cap = cap;
  return P;
}

// upload a host image into a zero-padded, 64-aligned-pitch scratch image
int upload_flat(orbx_ctx* c, DevBuf& b, const uint8_t* img, int w, int h, int stride, int* pitch) {
  const int p = align_up(w, 64);
  ENSURE(c, b, (size_t)p * h + 256);
  HIPCHK(c, hipMemsetAsync(b.p, 0, (size_t)p * h, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(b.p, p, img, stride, w, h, hipMemcpyHostToDevice, c->stream));
  *pitch = p;
  return ORBX_OK;
}

}  // namespace

// ===========================================================================
extern "C" {

int orbx_params_default_gpu(orbx_params* p) {
  if (!p) return ORBX_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  p->nfeatures = 500;  // include/orb.hpp:36
  p->scale_factor = 1.2f;
  p->nlevels = 8;
  p->threshold = 20;  // include/orb.hpp:12
  p->n = 9;
  p->nms_window = 3;
  p->patch_size = 31;
  p->harris_window = 7;  // src/orb.cpp:65
  p->harris_k = 0.04f;
  p->select_mode = ORBX_SELECT_HARRIS;
  p->blur_levels = ORBX_BLUR_NONE;
  p->blur_kind = ORBX_BLUR_SEP16;
  p->max_width = 1920;
  p->max_height = 1080;
  p->max_batch = 1;
  p->device = -1;
  return ORBX_OK;
}

int orbx_params_default_cpu(orbx_params* p) {
  int st = orbx_params_default_gpu(p);
  if (st != ORBX_OK) return st;
  p->nfeatures = 3000;  // include/orb_cpu.hpp:6
  p->threshold = 50;
  p->n = 9;
  p->nms_window = 3;
  p->patch_size = 9;
  p->nlevels = 1;  // ORBCPU::detectAndCompute ignores the pyramid (src/orb_cpu.cpp:271-276)
  p->select_mode = ORBX_SELECT_ROWMAJOR;
  return ORBX_OK;
}

const char* orbx_status_string(int status) {
  switch (status) {
    case ORBX_OK:
      return "ok";
    case ORBX_ERR_INVALID_ARG:
      return "invalid argument";
    case ORBX_ERR_CAPACITY:
      return "output capacity exceeded";
    case ORBX_ERR_HIP:
      return "HIP runtime error";
    case ORBX_ERR_NO_DEVICE:
      return "no usable gfx950 device";
    case ORBX_ERR_UNSUPPORTED:
      return "unsupported parameter combination";
    default:
      return "unknown status";
  }
}

const char* orbx_version(void) { return "liborbx 0.1.0 gfx950"; }

const char* orbx_last_error_string(const orbx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void orbx_destroy(orbx_ctx* c) {
  DeviceGuard _dg(c);
  if (!c) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->lanes[1].stream) (void)hipStreamSynchronize(c->lanes[1].stream);
  for (int i = 0; i < orbx_ctx::kGraphs; i++) drop_graph(c, i);
  for (Lane& L : c->lanes) {  // (the second lane of the pipelined mode: also what a failed enable left behind)
    free_lane(c, L);
    if (L.ev_pool) (void)hipEventDestroy(L.ev_pool);
  }
  for (TileTable& T : c->tiles)
    if (T.d) (void)hipFree(T.d);
  void* bufs[] = {c->d_in, c->d_taps, c->d_gauss, c->d_feedback};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c->h_feedback) (void)hipHostFree(const_cast<uint32_t*>(c->h_feedback));
  for (Block& B : c->blocks) {
    if (B.h) (void)hipHostFree(B.h);
    if (B.d) (void)hipFree(B.d);
    if (B.ev_done) (void)hipEventDestroy(B.ev_done);
    if (B.ev_copied) (void)hipEventDestroy(B.ev_copied);
  }
  if (c->cstream) {
    (void)hipStreamSynchronize(c->cstream);
    (void)hipStreamDestroy(c->cstream);
  }
  DevBuf* sb[] = {&c->s_img_a, &c->s_img_b, &c->s_f32,  &c->s_u16, &c->s_mask, &c->s_kps,   &c->s_f32b, &c->s_desc,
                  &c->s_i32,   &c->s_kern,  &c->s_tiles, &c->m_q,    &c->m_t,   &c->m_idx,  &c->m_dist,  &c->m_match, &c->m_cnt,
                  &c->lk_img[0], &c->lk_img[1], &c->lk_deriv, &c->lk_io, &c->pb_pts, &c->pb_n, &c->pb_out,
                  &c->pb_mask, &c->ph_in, &c->ph_pts, &c->ph_n, &c->ph_out, &c->ph_mask, &c->sb_xyz, &c->sb_valid,
                  &c->sb_mq, &c->sb_mt, &c->sb_n, &c->sb_out, &c->sh_in, &c->sh_xyz, &c->sh_valid, &c->sh_out,
                  &c->ba_off, &c->ba_poses, &c->ba_points, &c->ba_rows, &c->ba_opose, &c->ba_oxy, &c->ba_wp, &c->ba_wo,
                  &c->ba_slot, &c->ba_out, &c->gf_ws, &c->gf_img, &c->gf_res,
                  &c->lkw_ws, &c->lkw_first, &c->lkw_img, &c->lkw_pts, &c->lkw_res};
  if (c->gf_ev) {
    (void)hipEventSynchronize(c->gf_ev);
    (void)hipEventDestroy(c->gf_ev);
  }
  if (c->lkw_ev) {
    (void)hipEventSynchronize(c->lkw_ev);
    (void)hipEventDestroy(c->lkw_ev);
  }
  if (c->lkw_first_ev) (void)hipEventDestroy(c->lkw_first_ev);
  if (c->lkw_first_host) (void)hipHostFree(c->lkw_first_host);
  if (c->lk_host) (void)hipHostFree(c->lk_host);
  for (DevBuf* b : sb)
    if (b->p) (void)hipFree(b->p);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (TimingSet& set : c->evr)
    for (auto& e : set.ev)
      if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int orbx_create(const orbx_params* p, orbx_ctx** out) {
  if (!p || !out) return fail(nullptr, ORBX_ERR_INVALID_ARG, "params/out is NULL");
  *out = nullptr;
  std::string why;
  int st = validate_params(*p, &why);
  if (st != ORBX_OK) return fail(nullptr, st, why);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBX_ERR_NO_DEVICE, "hipGetDeviceCount found no device (liborbx has no CPU fallback)");
  int dev = p->device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  if (dev >= ndev) return fail(nullptr, ORBX_ERR_INVALID_ARG, "device ordinal out of range");
  DeviceGuard dg(dev);  // the caller's current device is restored on every return path
  {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != dev) return fail(nullptr, ORBX_ERR_NO_DEVICE, "hipSetDevice failed");
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
    return fail(nullptr, ORBX_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, ORBX_ERR_NO_DEVICE,
                std::string("device is ") + prop.gcnArchName + ", liborbx is built for gfx950 only");

  orbx_ctx* c = new (std::nothrow) orbx_ctx();
  if (!c) return fail(nullptr, ORBX_ERR_HIP, "out of host memory");
  c->p = *p;
  c->device = dev;

  c->fast_impl = fast_impl_env();
  c->blur_impl = blur_impl_env();
  st = build_plan(c->p, p->max_width, p->max_height, &c->plan_max, &why, c->fast_impl);
  if (st != ORBX_OK) {
    delete c;
    return fail(nullptr, st, why);
  }
  const OrbxPlan& M = c->plan_max;
  const size_t B = (size_t)p->max_batch;

#define CREATE_CHK(expr)                                                                     \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      std::string m = std::string(#expr) + ": " + hipGetErrorString(_e);                     \
      orbx_destroy(c);                                                                       \
      return fail(nullptr, ORBX_ERR_HIP, m);                                                 \
    }                                                                                        \
  } while (0)

  CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->lanes[0].stream = c->stream;  // lane 0 of the pipelined mode runs on the context's own stream
  for (auto& e : c->ev) CREATE_CHK(hipEventCreate(&e));
  for (TimingSet& set : c->evr)
    for (auto& e : set.ev) CREATE_CHK(hipEventCreate(&e));
  CREATE_CHK(hipMalloc((void**)&c->d_in, B * (size_t)p->max_width * p->max_height + 256));
  CREATE_CHK(alloc_lane_pools(c, c->lanes[0]));
  CREATE_CHK(hipMalloc((void**)&c->d_feedback, ORBX_FEEDBACK_WORDS * 4));
  CREATE_CHK(hipMemset(c->d_feedback, 0, ORBX_FEEDBACK_WORDS * 4));
  CREATE_CHK(hipHostMalloc((void**)&c->h_feedback, ORBX_FEEDBACK_WORDS * 4, hipHostMallocDefault));
  for (int i = 0; i < ORBX_FEEDBACK_WORDS; i++) c->h_feedback[i] = 0;
  OrbxTableCapacity tcap{};  // what any frame up to the maximum needs of the table pools (orbx_plan.h: table_capacity)
  if ((st = table_capacity(*p, M, c->fast_impl, c->blur_impl, &tcap, &why)) != ORBX_OK) {
    orbx_destroy(c);
    return fail(nullptr, st, why);
  }
  for (TileTable& T : c->tiles) T.capacity = tcap.frame;
  c->tiles[T_FAST].capacity = tcap.fast;
  c->tiles[T_PYRBLUR_SMALL].capacity = tcap.small;
  for (TileTable& T : c->tiles)
    CREATE_CHK(hipMalloc((void**)&T.d, std::max<size_t>(T.capacity, 1) * sizeof(OrbxTileDesc)));
  {
    // level sizes of smaller frames never exceed those of the largest frame
    c->taps_capacity = tcap.taps;
    CREATE_CHK(hipMalloc((void**)&c->d_taps, c->taps_capacity * sizeof(OrbxResizeTap)));
  }
  {
    const int K = p->harris_window;
    std::vector<float> g((size_t)K * K);
    gaussian_kernel(K, -1.0f, g.data());
    CREATE_CHK(hipMalloc((void**)&c->d_gauss, g.size() * sizeof(float)));
    CREATE_CHK(hipMemcpy(c->d_gauss, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  {
    const OutLayout o = make_out_layout((int)B, slots_per_frame(M));  // (the largest block any batch can need)
    {
      // The copy stream gets the HIGHEST priority -- not for the copies' sake: streams of one priority share a few
      // hardware queues, and the copy of a batch is enqueued behind a wait for the batch's end.  In a queue shared
      // with the other lane's stream that wait holds back the other lane's kernels for as long as the batch runs
      // (measured: the rate with the results on the host then falls from 0.99 to 0.8 of the rate without copies,
      // depending on which streams the process happens to have created); another priority is another queue.
      int least = 0, greatest = 0;
      CREATE_CHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      CREATE_CHK(hipStreamCreateWithPriority(&c->cstream, hipStreamNonBlocking, greatest));
    }
    for (Block& blk : c->blocks) {
      CREATE_CHK(hipMalloc((void**)&blk.d, o.total));
      CREATE_CHK(hipHostMalloc((void**)&blk.h, o.total, hipHostMallocDefault));
      CREATE_CHK(hipHostGetDevicePointer((void**)&blk.h_dev, blk.h, 0));
      CREATE_CHK(hipEventCreateWithFlags(&blk.ev_done, hipEventDisableTiming));
      CREATE_CHK(hipEventCreateWithFlags(&blk.ev_copied, hipEventDisableTiming));
    }
    for (Lane& L : c->lanes) CREATE_CHK(hipEventCreateWithFlags(&L.ev_pool, hipEventDisableTiming));
  }
#undef CREATE_CHK
  *out = c;
  return ORBX_OK;
}

int orbx_get_plan(orbx_ctx* c, int width, int height, int32_t* level_w, int32_t* level_h, int32_t* quota,
                  int32_t* fast_cap, float* level_scale_out, int32_t* out_capacity) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  OrbxPlan plan;
  std::string why;
  int st = build_plan(c->p, width, height, &plan, &why, c->fast_impl);
  if (st != ORBX_OK) return fail(c, st, why);
  for (int l = 0; l < plan.nlevels; l++) {
    if (level_w) level_w[l] = plan.L[l].w;
    if (level_h) level_h[l] = plan.L[l].h;
    if (quota) quota[l] = plan.L[l].quota;
    if (fast_cap) fast_cap[l] = plan.L[l].cap;
    if (level_scale_out) level_scale_out[l] = plan.L[l].scale;
  }
  if (out_capacity) *out_capacity = plan.out_cap;
  return ORBX_OK;
}

int orbx_detect_and_compute_batch_device(orbx_ctx* c, const void* d_frames, int n, int width, int height,
                                         int row_stride, size_t frame_stride, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!d_frames) return fail(c, ORBX_ERR_INVALID_ARG, "d_frames is NULL");
  if (n < 1 || n > c->p.max_batch) return fail(c, ORBX_ERR_INVALID_ARG, "n outside [1, max_batch]");
  if (row_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "row_stride < width");
  if (frame_stride < (size_t)row_stride * (size_t)(height - 1) + (size_t)width)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame_stride smaller than a frame");
  // the kernels address the bytes of one frame with 32-bit offsets (a buffer descriptor per frame)
  if ((unsigned long long)row_stride * (unsigned long long)(height - 1) + (unsigned long long)width > 0x7fffffffull)
    return fail(c, ORBX_ERR_INVALID_ARG, "row_stride * (height - 1) + width exceeds 2^31 - 1");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return run_batch(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride, s, true);
}

int orbx_detect_and_compute_batch_host(orbx_ctx* c, const uint8_t* frames, int n, int width, int height,
                                       int row_stride, size_t frame_stride) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 1 || n > c->p.max_batch) return fail(c, ORBX_ERR_INVALID_ARG, "n outside [1, max_batch]");
  int st = check_image(c, frames, width, height, row_stride);
  if (st != ORBX_OK) return st;
  if (n > 1 && frame_stride < (size_t)row_stride * (size_t)(height - 1) + (size_t)width)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame_stride smaller than a frame");
  const size_t tight = (size_t)width * height;
  if (row_stride == width && (n == 1 || frame_stride == tight)) {
    HIPCHK(c, hipMemcpyAsync(c->d_in, frames, tight * n, hipMemcpyHostToDevice, c->stream));
  } else {
    for (int i = 0; i < n; i++)
      HIPCHK(c, hipMemcpy2DAsync(c->d_in + tight * i, width, frames + frame_stride * i, row_stride, width, height,
                                 hipMemcpyHostToDevice, c->stream));
  }
  return run_batch(c, c->d_in, n, width, height, width, tight, c->stream);
}

int orbx_wait(orbx_ctx* c) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  HIPCHK(c, hipStreamSynchronize(batch_stream(c)));
  HIPCHK(c, lanes_sync(c));
  return ORBX_OK;
}

int orbx_set_host_results(orbx_ctx* c, int enable) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  c->host_results = enable ? 1 : 0;  // (takes effect with the next batched call: part of the launch sequence's key)
  return ORBX_OK;
}

int orbx_set_pipelined_batches(orbx_ctx* c, int enable) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->last_stream) HIPCHK(c, hipStreamSynchronize(c->last_stream));
  HIPCHK(c, lanes_sync(c));
  Lane& L = c->lanes[1];
  if (enable && !L.stream) {  // the second lane: a stream and a second set of working pools
    hipError_t e = alloc_lane_pools(c, L);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
    if (e != hipSuccess) {  // (at batch 512 the second pool set is GBs: running out of memory is the realistic failure)
      free_lane(c, L);
      c->pipelined = false;
      return fail(c, ORBX_ERR_HIP, std::string("second lane of the pipelined mode: ") + hipGetErrorString(e));
    }
  }
  c->pipelined = enable != 0;
  return ORBX_OK;
}

// Debug entry (tests): every working pool of both lanes is filled with `byte`, so that a kernel that consumes a word
// an earlier batch, another frame size or another tile partition left behind shows in the results.
int orbx_debug_fill_pools(orbx_ctx* c, int byte) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (byte < 0 || byte > 255) return fail(c, ORBX_ERR_INVALID_ARG, "byte must be in [0, 255]");
  if (c->last_stream) HIPCHK(c, hipStreamSynchronize(c->last_stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, lanes_sync(c));
  for (Lane& L : c->lanes) {
    if (!L.d_mask) continue;  // (lane 1 exists once the pipelined mode has been switched on)
    for (const PoolRef& r : lane_pools(c, L))
      if (*r.p && *r.p != L.d_pyr_blur) HIPCHK(c, hipMemsetAsync(*r.p, byte, r.bytes, c->stream));
    // The blurred pyramid is the one pool that must hold zeroes: the padding bytes of its levels (set_plan zeroes
    // them, the fused pyramid + blur kernel never writes them, BRIEF reads them as the zero extension of a row).  So
    // only the PIXELS of the current plan's levels are filled -- what a skipped strip of the top-rows-first pipeline
    // leaves behind -- and nothing before a plan is set.
    if (L.d_pyr_blur && c->plan_w > 0)
      for (size_t f = 0; f < (size_t)c->p.max_batch; f++)
        for (int l = 0; l < c->plan.nlevels; l++) {
          const OrbxLevel& V = c->plan.L[l];
          HIPCHK(c, hipMemset2DAsync(L.d_pyr_blur + f * (size_t)c->plan.frame_bytes + (size_t)V.img_off, (size_t)V.pitch, byte,
                                     (size_t)V.w, (size_t)V.h, c->stream));
        }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_set_fast_early_exit(orbx_ctx* c, int enable) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  c->fast_early = enable != 0;
  return ORBX_OK;
}

int orbx_set_fused_pyramid_blur(orbx_ctx* c, int enable) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  c->fuse = enable != 0;
  return ORBX_OK;
}

int orbx_set_top_rows_first(orbx_ctx* c, int mode) {
  DeviceGuard _dg(c);
  if (!c || mode < 0 || mode > 2) return ORBX_ERR_INVALID_ARG;
  c->top_mode = mode;
  c->top_on = true;
  c->top_single_batches = 0;
  return ORBX_OK;
}

int orbx_fast_tile_counts(orbx_ctx* c, long long* worked, long long* total) {
  DeviceGuard _dg(c);
  if (!c || !worked || !total) return ORBX_ERR_INVALID_ARG;
  if (c->plan_w == 0 || last_block(c).n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "run a batch first");
  const int n = last_block(c).n;
  std::vector<unsigned long long> h((size_t)n * ORBX_FAST_STAT_WORDS);
  HIPCHK(c, hipStreamSynchronize(c->last_stream));
  HIPCHK(c, hipMemcpy(h.data(), cur_lane(c).d_row_stat, h.size() * 8, hipMemcpyDeviceToHost));
  long long w = 0;
  for (int f = 0; f < n; f++)
    for (int l = 0; l < c->plan.nlevels; l++)
      for (int b = 0; b < c->bm_fast.tiles_y[l]; b++)
        w += (long long)(h[(size_t)f * ORBX_FAST_STAT_WORDS + (size_t)l * ORBX_MAX_BANDS + b] >> 32);
  *total = (long long)c->bm_fast.band_begin[c->bm_fast.nbands] * n;
  *worked = fast_early_on(c) ? w : *total;  // (no statistics are kept when the early exit is off)
  return ORBX_OK;
}

int orbx_pyramid_pixel_counts(orbx_ctx* c, long long* produced, long long* total) {
  DeviceGuard _dg(c);
  if (!c || !produced || !total) return ORBX_ERR_INVALID_ARG;
  if (c->plan_w == 0 || last_block(c).n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "run a batch first");
  const int n = last_block(c).n, top = top_rows_env();
  long long per_frame = 0;
  for (int l = 0; l < c->plan.nlevels; l++) per_frame += (long long)c->plan.L[l].w * c->plan.L[l].h;
  *total = per_frame * n;
  *produced = *total;
  if (!c->last_two_pass) return ORBX_OK;
  std::vector<unsigned long long> h((size_t)n * ORBX_FAST_STAT_WORDS);
  HIPCHK(c, hipStreamSynchronize(c->last_stream));
  HIPCHK(c, hipMemcpy(h.data(), cur_lane(c).d_row_stat, h.size() * 8, hipMemcpyDeviceToHost));
  long long done = 0;
  for (int f = 0; f < n; f++)
    for (int l = 0; l < c->plan.nlevels; l++) {
      const OrbxLevel& L = c->plan.L[l];
      const int first = pyrblur_first_pass_rows(c->plan, c->bm_fast, l, top);
      long long surv = 0;  // the kernel's test: survivors of the first-pass tile rows
      for (int b = 0; b < std::min(top, c->bm_fast.tiles_y[l]); b++)
        surv += (long long)(uint32_t)h[(size_t)f * ORBX_FAST_STAT_WORDS + (size_t)l * ORBX_MAX_BANDS + b];
      done += (long long)L.w * (first < L.h && surv >= L.cap ? first : L.h);
    }
  *produced = done;
  return ORBX_OK;
}

int orbx_enable_stage_timing(orbx_ctx* c, int enable) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  c->timing = enable < 0 || enable > 2 ? 1 : enable;
  return ORBX_OK;
}

int orbx_stage_times_history(orbx_ctx* c, int back, float* ms) {
  DeviceGuard _dg(c);
  if (!c || !ms) return ORBX_ERR_INVALID_ARG;
  if (back < 0 || back >= ORBX_EVENT_SETS || back >= c->ev_calls)
    return fail(c, ORBX_ERR_INVALID_ARG, "no timed batched call that far back");
  const long long call = c->ev_calls - 1 - back;
  const TimingSet& ts = c->evr[call % ORBX_EVENT_SETS];
  const hipEvent_t* evs = ts.ev;
  const int mode = ts.mode;
  std::memset(ms, 0, sizeof(float) * ORBX_NUM_STAGE_TIMES);
  if (mode == 1) {
    for (int i = 0; i < ORBX_NUM_STAGE_TIMES - 1; i++) HIPCHK(c, hipEventElapsedTime(&ms[i], evs[i], evs[i + 1]));
    HIPCHK(c, hipEventElapsedTime(&ms[ORBX_NUM_STAGE_TIMES - 1], evs[0], evs[ORBX_NUM_STAGE_TIMES - 1]));
  } else {  // blur and fast+nms only
    HIPCHK(c, hipEventElapsedTime(&ms[1], evs[1], evs[2]));
    HIPCHK(c, hipEventElapsedTime(&ms[2], evs[2], evs[3]));
  }
  if (ts.split) {
    // top-rows-first pipeline: events 1 | pyramid+blur (top) | N+1 | FAST (top) | N+2 | pyramid+blur (rest) | 2 | FAST (rest) | 3
    float a = 0, b = 0, d = 0, e = 0;
    HIPCHK(c, hipEventElapsedTime(&a, evs[1], evs[ORBX_NUM_STAGE_TIMES + 1]));
    HIPCHK(c, hipEventElapsedTime(&b, evs[ORBX_NUM_STAGE_TIMES + 1], evs[ORBX_NUM_STAGE_TIMES + 2]));
    HIPCHK(c, hipEventElapsedTime(&d, evs[ORBX_NUM_STAGE_TIMES + 2], evs[2]));
    HIPCHK(c, hipEventElapsedTime(&e, evs[2], evs[3]));
    ms[1] = a + d;
    ms[2] = b + e;
  }
  return ORBX_OK;
}

int orbx_last_stage_times(orbx_ctx* c, float* ms) { return orbx_stage_times_history(c, 0, ms); }

int orbx_batch_results_device(orbx_ctx* c, orbx_batch_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const Block& B = last_block(c);
  if (B.n <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been run");
  const OutLayout& o = B.layout;
  v->counts = (const int32_t*)(B.d + o.counts);
  v->keypoints = (const orbx_keypoint*)(B.d + o.kp);
  v->keypoints16 = (const uint32_t*)(B.d + o.kp16);
  v->level_kps = (const orbx_keypoint*)(B.d + o.lkp);
  v->orientations = (const float*)(B.d + o.angle);
  v->responses = (const float*)(B.d + o.resp);
  v->levels = (const int32_t*)(B.d + o.level);
  v->descriptors = (const orbx_descriptor*)(B.d + o.desc);
  v->slot_capacity = B.cap;
  v->n = B.n;
  return ORBX_OK;
}

namespace {
// frames [first, first+n) of result block `b` -> host arrays.  If an asynchronous copy of the block
// is pending (orbx_batch_prefetch) only its event is waited for; otherwise ONE blocking D2H of the block.
int fetch_block(orbx_ctx* c, int b, int first, int n, int32_t* counts, orbx_keypoint* keypoints, float* orientations,
                orbx_descriptor* descriptors, float* responses, int32_t* levels, orbx_keypoint* level_kps,
                int capacity) {
  Block& B = c->blocks[b];
  if (!counts) return fail(c, ORBX_ERR_INVALID_ARG, "counts is NULL");
  if (first < 0 || n < 1 || first + n > B.n) return fail(c, ORBX_ERR_INVALID_ARG, "frame range outside batch");
  if (capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "capacity < 0");
  const OutLayout& o = B.layout;
  const int cap = B.cap;
  const uint8_t* h = B.h;
  if (B.copy_pending && B.copy_compact && (responses || levels || level_kps)) {
    // only the compact prefix is on its way: fetch the other sections now (blocking)
    HIPCHK(c, hipEventSynchronize(B.ev_copied));
    HIPCHK(c, hipMemcpyAsync(B.h + o.compact, B.d + o.compact, o.total - o.compact, hipMemcpyDeviceToHost,
                             c->cstream));
    HIPCHK(c, hipStreamSynchronize(c->cstream));
    B.copy_compact = false;
  } else if (B.copy_pending) {
    HIPCHK(c, hipEventSynchronize(B.ev_copied));
  } else if (b == c->blk) {
    // blocking fetch of the last batch: the copy goes behind the batch on ITS stream (no hop to the copy
    // stream: the synchronous one-frame call is latency-bound)
    hipStream_t s = batch_stream(c);
    HIPCHK(c, hipMemcpyAsync(B.h, B.d, o.total, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  } else {
    HIPCHK(c, hipStreamWaitEvent(c->cstream, B.ev_done, 0));
    HIPCHK(c, hipMemcpyAsync(B.h, B.d, o.total, hipMemcpyDeviceToHost, c->cstream));
    HIPCHK(c, hipStreamSynchronize(c->cstream));
  }
  const int32_t* hc = (const int32_t*)(h + o.counts);
  bool truncated = false;
  for (int i = 0; i < n; i++) {
    const int f = first + i;
    const int cnt = hc[f];
    counts[i] = cnt;
    const int m = std::min(cnt, capacity);
    if (cnt > capacity) truncated = true;
    const size_t so = (size_t)f * cap, dst = (size_t)i * capacity;
    if (keypoints) {  // (a compact copy holds them packed only: x | y << 16)
      const uint32_t* k16 = (const uint32_t*)(h + o.kp16) + so;
      for (int j = 0; j < m; j++) keypoints[dst + j] = orbx_keypoint{(int32_t)(k16[j] & 0xffffu), (int32_t)(k16[j] >> 16)};
    }
    if (level_kps) std::memcpy(level_kps + dst, (const orbx_keypoint*)(h + o.lkp) + so, sizeof(orbx_keypoint) * m);
    if (orientations) std::memcpy(orientations + dst, (const float*)(h + o.angle) + so, sizeof(float) * m);
    if (responses) std::memcpy(responses + dst, (const float*)(h + o.resp) + so, sizeof(float) * m);
    if (levels) std::memcpy(levels + dst, (const int32_t*)(h + o.level) + so, sizeof(int32_t) * m);
    if (descriptors)
      std::memcpy(descriptors + dst, (const orbx_descriptor*)(h + o.desc) + so, sizeof(orbx_descriptor) * m);
  }
  if (truncated) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than keypoint count");
  return ORBX_OK;
}
}  // namespace

int orbx_batch_fetch(orbx_ctx* c, int first, int n, int32_t* counts, orbx_keypoint* keypoints,
                     float* orientations, orbx_descriptor* descriptors, float* responses, int32_t* levels,
                     orbx_keypoint* level_kps, int capacity) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return fetch_block(c, c->blk, first, n, counts, keypoints, orientations, descriptors, responses, levels, level_kps,
                     capacity);
}

int orbx_batch_results_host(orbx_ctx* c, int previous, orbx_batch_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (previous < 0 || previous >= orbx_ctx::kBlocks) return fail(c, ORBX_ERR_INVALID_ARG, "previous must be 0..3 (a ring of four result blocks)");
  Block& B = c->blocks[(c->blk + orbx_ctx::kBlocks - previous) % orbx_ctx::kBlocks];
  if (B.n <= 0) return fail(c, ORBX_ERR_INVALID_ARG, previous ? "there is no batch that far back" : "no batch has been run");
  const OutLayout& o = B.layout;
  if (B.copy_pending) {
    HIPCHK(c, hipEventSynchronize(B.ev_copied));
  } else {
    HIPCHK(c, hipStreamWaitEvent(c->cstream, B.ev_done, 0));
    HIPCHK(c, hipMemcpyAsync(B.h, B.d, o.total, hipMemcpyDeviceToHost, c->cstream));
    HIPCHK(c, hipEventRecord(B.ev_copied, c->cstream));
    B.copy_pending = true;
    HIPCHK(c, hipEventSynchronize(B.ev_copied));
  }
  const uint8_t* h = B.h;
  const bool compact = B.copy_compact;  // (those sections of the mirror were not copied: NULL in the view)
  v->counts = (const int32_t*)(h + o.counts);
  v->keypoints = compact ? nullptr : (const orbx_keypoint*)(h + o.kp);
  v->keypoints16 = (const uint32_t*)(h + o.kp16);
  v->level_kps = compact ? nullptr : (const orbx_keypoint*)(h + o.lkp);
  v->orientations = (const float*)(h + o.angle);
  v->responses = compact ? nullptr : (const float*)(h + o.resp);
  v->levels = compact ? nullptr : (const int32_t*)(h + o.level);
  v->descriptors = (const orbx_descriptor*)(h + o.desc);
  v->slot_capacity = B.cap;
  v->n = B.n;
  return ORBX_OK;
}

namespace {
int prefetch_block(orbx_ctx* c, bool compact) {
  Block& B = c->blocks[c->blk];
  if (B.n <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been run");
  const OutLayout& o = B.layout;
  if (B.copy_pending) {
    if (compact || !B.copy_compact) return ORBX_OK;
    // a compact copy is on its way and the whole block is wanted after all: the other sections follow it
    HIPCHK(c, hipStreamWaitEvent(c->cstream, B.ev_done, 0));  // (host results: the compact part never was on this stream)
    HIPCHK(c, hipMemcpyAsync(B.h + o.compact, B.d + o.compact, o.total - o.compact, hipMemcpyDeviceToHost,
                             c->cstream));
    HIPCHK(c, hipEventRecord(B.ev_copied, c->cstream));
    B.copy_compact = false;
    return ORBX_OK;
  }
  // (a block the describe kernel has written its compact record into -- orbx_set_host_results -- never gets here:
  // it is compact-pending from the moment the batch is enqueued)
  HIPCHK(c, hipStreamWaitEvent(c->cstream, B.ev_done, 0));
  HIPCHK(c, hipMemcpyAsync(B.h, B.d, compact ? o.compact : o.total, hipMemcpyDeviceToHost, c->cstream));
  HIPCHK(c, hipEventRecord(B.ev_copied, c->cstream));
  B.copy_pending = true;
  B.copy_compact = compact;
  return ORBX_OK;
}
}  // namespace

int orbx_batch_prefetch(orbx_ctx* c) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return prefetch_block(c, false);
}

int orbx_batch_prefetch_compact(orbx_ctx* c) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return prefetch_block(c, true);
}

int orbx_batch_fetch_previous(orbx_ctx* c, int first, int n, int32_t* counts, orbx_keypoint* keypoints,
                              float* orientations, orbx_descriptor* descriptors, float* responses, int32_t* levels,
                              orbx_keypoint* level_kps, int capacity) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int b = (c->blk + orbx_ctx::kBlocks - 1) % orbx_ctx::kBlocks;
  if (c->blocks[b].n <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "there is no batch before the last one");
  return fetch_block(c, b, first, n, counts, keypoints, orientations, descriptors, responses, levels, level_kps,
                     capacity);
}

int orbx_detect_and_compute(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                            orbx_keypoint* keypoints, float* orientations, orbx_descriptor* descriptors,
                            float* responses, int32_t* levels, orbx_keypoint* level_kps, int capacity,
                            int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count) return fail(c, ORBX_ERR_INVALID_ARG, "count is NULL");
  int st = orbx_detect_and_compute_batch_host(c, image, 1, width, height, stride, (size_t)stride * height);
  if (st != ORBX_OK) return st;
  int32_t cnt = 0;
  st = orbx_batch_fetch(c, 0, 1, &cnt, keypoints, orientations, descriptors, responses, levels, level_kps,
                        capacity);
  *count = cnt;
  return st;
}

int orbx_bench_stage(orbx_ctx* c, int n_frames, int stage, int reps, float* avg_ms) {
  DeviceGuard _dg(c);
  if (!c || !avg_ms) return ORBX_ERR_INVALID_ARG;
  if (c->plan_w == 0) return fail(c, ORBX_ERR_INVALID_ARG, "run a batch first (no pyramid built)");
  if (n_frames < 1 || n_frames > last_block(c).n || reps < 1) return fail(c, ORBX_ERR_INVALID_ARG, "n_frames/reps");
  const OrbxPlan& P = c->plan;
  const Lane& L = cur_lane(c);
  hipStream_t s = c->stream;
  OrbxFastParams fp{c->p.threshold, c->p.n, c->p.nms_window / 2};
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, lanes_sync(c));  // (the last batch may have run on the other lane's stream)
  HIPCHK(c, hipEventRecord(c->ev[0], s));
  for (int i = 0; i < reps; i++) {
    switch (stage) {
      case ORBX_STAGE_BLUR:
        if (!blur_enabled(c)) return fail(c, ORBX_ERR_INVALID_ARG, "blur is disabled in this context");
        HIPCHK(c, launch_blur_auto(c->blur_impl, s, P, c->tm_blur, c->tiles[T_BLUR].d, c->tiles[T_BLUR].count, n_frames,
                                   L.d_pyr, L.d_pyr_blur, c->p.blur_levels == ORBX_BLUR_UPPER ? 1 : 0, c->p.blur_kind));
        break;
      case ORBX_STAGE_FAST:
        HIPCHK(c, launch_fast_whole(c, s, n_frames, fp));
        break;
      case ORBX_STAGE_COMPACT:
        HIPCHK(c, orbx_launch_compact(s, P, n_frames, L.d_mask, L.d_cand, L.d_cand_count, L.d_cand_total, 0));
        break;
      default:
        return fail(c, ORBX_ERR_INVALID_ARG, "stage not benchmarkable in isolation");
    }
  }
  HIPCHK(c, hipEventRecord(c->ev[1], s));
  HIPCHK(c, hipEventSynchronize(c->ev[1]));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  *avg_ms = ms / reps;
  return ORBX_OK;
}

// ---- stage-level operators --------------------------------------------------

int orbx_fast_score(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int threshold, int n,
                    float* scores) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!scores || n < 1 || n > 16 || threshold < 0 || threshold > 255)
    return fail(c, ORBX_ERR_INVALID_ARG, "scores NULL or n/threshold out of range");
  int pitch;
  st = upload_flat(c, c->s_img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, 0);
  OrbxBandMap bm;
  std::string why;
  if ((st = make_bandmap(P, 0, &bm, &why)) != ORBX_OK) return fail(c, st, why);
  std::vector<OrbxTileDesc> t;
  build_fast_tiles(P, bm, 0, 1, &t);
  ENSURE(c, c->s_tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s_tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  const size_t npx = (size_t)width * height;
  ENSURE(c, c->s_u16, npx * 2);
  ENSURE(c, c->s_mask, (size_t)P.mask_words * 8);
  OrbxFastParams fp{threshold, n, 0};
  HIPCHK(c, orbx_launch_fast_nms(c->stream, (const OrbxTileDesc*)c->s_tiles.p, (int)t.size(), 1,
                                 (const uint8_t*)c->s_img_a.p, P.frame_bytes, P.mask_words, fp,
                                 (unsigned long long*)c->s_mask.p, (uint16_t*)c->s_u16.p, nullptr));
  std::vector<uint16_t> h(npx);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->s_u16.p, npx * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < npx; i++) scores[i] = (float)h[i];
  return ORBX_OK;
}

static int compact_and_fetch(orbx_ctx* c, const OrbxPlan& P, int nfeatures, orbx_keypoint* keypoints, int* count,
                             int* total) {
  ENSURE(c, c->s_kps, sizeof(orbx_keypoint) * (size_t)std::max(nfeatures, 1));
  ENSURE(c, c->s_i32, 64);
  int32_t* d_cnt = (int32_t*)c->s_i32.p;
  HIPCHK(c, orbx_launch_compact(c->stream, P, 1, (const unsigned long long*)c->s_mask.p, (orbx_keypoint*)c->s_kps.p,
                                d_cnt, d_cnt + 1, 1));
  int32_t h[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[0] > 0)
    HIPCHK(c, hipMemcpy(keypoints, c->s_kps.p, sizeof(orbx_keypoint) * (size_t)h[0], hipMemcpyDeviceToHost));
  *count = h[0];
  if (total) *total = h[1];
  return ORBX_OK;
}

int orbx_fast(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int threshold, int n,
              int nms_window, int nfeatures, orbx_keypoint* keypoints, int* count, int* total) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!count || (!keypoints && nfeatures > 0) || nfeatures < 0 || n < 1 || n > 16 || threshold < 0 ||
      threshold > 255 || nms_window < 0 || nms_window / 2 > 3)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad Fast() arguments");
  int pitch;
  st = upload_flat(c, c->s_img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, nfeatures);
  OrbxBandMap bm;
  std::string why;
  if ((st = make_bandmap(P, nms_window / 2, &bm, &why)) != ORBX_OK) return fail(c, st, why);
  std::vector<OrbxTileDesc> t;
  build_fast_tiles(P, bm, 0, 1, &t);
  ENSURE(c, c->s_tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s_tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  ENSURE(c, c->s_mask, (size_t)P.mask_words * 8);
  OrbxFastParams fp{threshold, n, nms_window / 2};
  // stage operator: exact totals are part of the contract -> no early exit
  HIPCHK(c, orbx_launch_fast_nms(c->stream, (const OrbxTileDesc*)c->s_tiles.p, (int)t.size(), 1,
                                 (const uint8_t*)c->s_img_a.p, P.frame_bytes, P.mask_words, fp,
                                 (unsigned long long*)c->s_mask.p, nullptr, nullptr));
  return compact_and_fetch(c, P, nfeatures, keypoints, count, total);
}

int orbx_nms(orbx_ctx* c, const float* scores, int width, int height, int nms_window, int nfeatures,
             float threshold, orbx_keypoint* keypoints, int* count, int* total) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!scores || !count || (!keypoints && nfeatures > 0) || nfeatures < 0 || width < 1 || height < 1 ||
      nms_window < 0 || nms_window / 2 > 3)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad NMS() arguments");
  const size_t npx = (size_t)width * height;
  ENSURE(c, c->s_f32, npx * 4);
  OrbxPlan P = flat_plan(width, height, nfeatures);
  ENSURE(c, c->s_mask, (size_t)P.mask_words * 8);
  HIPCHK(c, hipMemcpyAsync(c->s_f32.p, scores, npx * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_nms_f32(c->stream, (const float*)c->s_f32.p, width, height, nms_window / 2, threshold,
                                (unsigned long long*)c->s_mask.p, P.L[0].mask_wpr));
  return compact_and_fetch(c, P, nfeatures, keypoints, count, total);
}

static int describe_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                          const orbx_keypoint* keypoints, int nkp, int patch_size, const float* angles_in,
                          float* angles_out, orbx_descriptor* desc_out) {
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (nkp < 0 || (nkp > 0 && !keypoints)) return fail(c, ORBX_ERR_INVALID_ARG, "keypoints NULL / nkp < 0");
  if (patch_size < 1 || patch_size / 2 > 20) return fail(c, ORBX_ERR_INVALID_ARG, "patch_size must be in [1, 41]");
  if (nkp == 0) return ORBX_OK;
  for (int i = 0; i < nkp; i++)
    if (keypoints[i].x < 0 || keypoints[i].y < 0 || keypoints[i].x >= width || keypoints[i].y >= height)
      return fail(c, ORBX_ERR_INVALID_ARG, "keypoint outside the image");
  if (angles_in)
    for (int i = 0; i < nkp; i++)
      if (!(std::fabs(angles_in[i]) < 100.0f))
        return fail(c, ORBX_ERR_INVALID_ARG, "orientation must be finite and |angle| < 100 rad");
  int pitch;
  st = upload_flat(c, c->s_img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  ENSURE(c, c->s_kps, sizeof(orbx_keypoint) * (size_t)nkp);
  ENSURE(c, c->s_f32b, sizeof(float) * (size_t)nkp);
  ENSURE(c, c->s_desc, sizeof(orbx_descriptor) * (size_t)nkp);
  HIPCHK(c, hipMemcpyAsync(c->s_kps.p, keypoints, sizeof(orbx_keypoint) * (size_t)nkp, hipMemcpyHostToDevice,
                           c->stream));
  if (angles_in)
    HIPCHK(c, hipMemcpyAsync(c->s_f32b.p, angles_in, sizeof(float) * (size_t)nkp, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_describe_flat(c->stream, (const uint8_t*)c->s_img_a.p, width, height, pitch,
                                      (const orbx_keypoint*)c->s_kps.p, nkp, patch_size, angles_in != nullptr,
                                      desc_out != nullptr, (float*)c->s_f32b.p, (orbx_descriptor*)c->s_desc.p));
  if (angles_out)
    HIPCHK(c, hipMemcpyAsync(angles_out, c->s_f32b.p, sizeof(float) * (size_t)nkp, hipMemcpyDeviceToHost, c->stream));
  if (desc_out)
    HIPCHK(c, hipMemcpyAsync(desc_out, c->s_desc.p, sizeof(orbx_descriptor) * (size_t)nkp, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_orientations(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                      const orbx_keypoint* keypoints, int nkp, int patch_size, float* orientations) {
  DeviceGuard _dg(c);
  if (c && nkp > 0 && !orientations) return fail(c, ORBX_ERR_INVALID_ARG, "orientations is NULL");
  return describe_stage(c, image, width, height, stride, keypoints, nkp, patch_size, nullptr, orientations, nullptr);
}

int orbx_brief(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
               const orbx_keypoint* keypoints, const float* orientations, int nkp, orbx_descriptor* descriptors) {
  DeviceGuard _dg(c);
  if (c && nkp > 0 && (!orientations || !descriptors))
    return fail(c, ORBX_ERR_INVALID_ARG, "orientations/descriptors is NULL");
  return describe_stage(c, image, width, height, stride, keypoints, nkp, 31, orientations, nullptr, descriptors);
}

int orbx_harris(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                const orbx_keypoint* keypoints, int nkp, int window, float k, float* responses) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (nkp < 0 || (nkp > 0 && (!keypoints || !responses)) || window < 1 || (window % 2) == 0 || window > 15)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad HarrisScore() arguments");
  if (nkp == 0) return ORBX_OK;
  for (int i = 0; i < nkp; i++)
    if (keypoints[i].x < 0 || keypoints[i].y < 0 || keypoints[i].x >= width || keypoints[i].y >= height)
      return fail(c, ORBX_ERR_INVALID_ARG, "keypoint outside the image");
  int pitch;
  st = upload_flat(c, c->s_img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  std::vector<float> g((size_t)window * window);
  gaussian_kernel(window, -1.0f, g.data());
  ENSURE(c, c->s_kern, g.size() * 4);
  ENSURE(c, c->s_kps, sizeof(orbx_keypoint) * (size_t)nkp);
  ENSURE(c, c->s_f32b, sizeof(float) * (size_t)nkp);
  HIPCHK(c, hipMemcpyAsync(c->s_kern.p, g.data(), g.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->s_kps.p, keypoints, sizeof(orbx_keypoint) * (size_t)nkp, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, orbx_launch_harris_flat(c->stream, (const uint8_t*)c->s_img_a.p, width, height, pitch,
                                    (const orbx_keypoint*)c->s_kps.p, nkp, (const float*)c->s_kern.p, window, k,
                                    (float*)c->s_f32b.p));
  HIPCHK(c, hipMemcpyAsync(responses, c->s_f32b.p, sizeof(float) * (size_t)nkp, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

static int blur_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                      int dst_stride, int kind) {
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!dst || dst_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "dst NULL or dst_stride < width");
  int pitch;
  st = upload_flat(c, c->s_img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, 0);
  ENSURE(c, c->s_img_b, (size_t)P.frame_bytes + 256);
  OrbxTileMap tm;
  make_tilemap(P, ORBX_BLUR_TW, ORBX_BLUR_TH, true, &tm);
  std::vector<OrbxTileDesc> t;
  blur_tiles_for_impl(c->blur_impl, P, &t);
  ENSURE(c, c->s_tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s_tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  HIPCHK(c, launch_blur_auto(c->blur_impl, c->stream, P, tm, (const OrbxTileDesc*)c->s_tiles.p, (int)t.size(), 1,
                             (const uint8_t*)c->s_img_a.p, (uint8_t*)c->s_img_b.p, 0, kind));
  HIPCHK(c, hipMemcpy2DAsync(dst, dst_stride, c->s_img_b.p, pitch, width, height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_blur5_sep(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride) {
  DeviceGuard _dg(c);
  return blur_stage(c, image, width, height, stride, dst, dst_stride, ORBX_BLUR_SEP16);
}

int orbx_blur5_273(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride) {
  DeviceGuard _dg(c);
  return blur_stage(c, image, width, height, stride, dst, dst_stride, ORBX_BLUR_K273);
}

static int conv_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, const float* kernel,
                      int K, int reflect_pad, uint8_t* dst) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!image || !kernel || !dst || width < 1 || height < 1 || stride < width || K < 1 || (K % 2) == 0 || K > 31)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad conv2d() arguments (kernel_size must be odd, <= 31)");
  const int wo = reflect_pad ? width : width - K + 1, ho = reflect_pad ? height : height - K + 1;
  if (wo < 1 || ho < 1) return fail(c, ORBX_ERR_INVALID_ARG, "image smaller than the kernel");
  if (reflect_pad && (width < K / 2 + 1 || height < K / 2 + 1))
    return fail(c, ORBX_ERR_INVALID_ARG, "image too small for REFLECT_101 padding");
  int pitch;
  const int p = align_up(width, 64);
  ENSURE(c, c->s_img_a, (size_t)p * height + 256);
  HIPCHK(c, hipMemcpy2DAsync(c->s_img_a.p, p, image, stride, width, height, hipMemcpyHostToDevice, c->stream));
  pitch = p;
  ENSURE(c, c->s_img_b, (size_t)wo * ho + 256);
  ENSURE(c, c->s_kern, (size_t)K * K * 4);
  HIPCHK(c, hipMemcpyAsync(c->s_kern.p, kernel, (size_t)K * K * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_conv2d(c->stream, (const uint8_t*)c->s_img_a.p, width, height, pitch,
                               (const float*)c->s_kern.p, K, reflect_pad, (uint8_t*)c->s_img_b.p, wo));
  HIPCHK(c, hipMemcpyAsync(dst, c->s_img_b.p, (size_t)wo * ho, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_conv2d(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, const float* kernel,
                int kernel_size, uint8_t* dst) {
  DeviceGuard _dg(c);
  return conv_stage(c, image, width, height, stride, kernel, kernel_size, 0, dst);
}

int orbx_gaussian_kernel(int kernel_size, float sigma, float* kernel) {
  return gaussian_kernel(kernel_size, sigma, kernel);
}

int orbx_gaussian_blur_conv(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int kernel_size,
                            uint8_t* dst) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (kernel_size < 1 || (kernel_size % 2) == 0 || kernel_size > 31)
    return fail(c, ORBX_ERR_INVALID_ARG, "kernel_size must be odd and <= 31 (src/GaussianBlur.cpp:8-11)");
  std::vector<float> g((size_t)kernel_size * kernel_size);
  gaussian_kernel(kernel_size, -1.0f, g.data());
  return conv_stage(c, image, width, height, stride, g.data(), kernel_size, 1, dst);
}

int orbx_sobel(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int dir, uint8_t* dst) {
  DeviceGuard _dg(c);
  static const float SX[9] = {-1.f, 0.f, 1.f, -2.f, 0.f, 2.f, -1.f, 0.f, 1.f};   // src/Sobel.cpp:6-10
  static const float SY[9] = {-1.f, -2.f, -1.f, 0.f, 0.f, 0.f, 1.f, 2.f, 1.f};   // src/Sobel.cpp:12-16
  return conv_stage(c, image, width, height, stride, dir == 0 ? SX : SY, 3, 1, dst);
}

int orbx_build_pyramid_level(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int level,
                             uint8_t* dst, int* level_w, int* level_h) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (level < 0 || level >= c->p.nlevels || !dst) return fail(c, ORBX_ERR_INVALID_ARG, "level out of range / dst NULL");
  if ((st = set_plan(c, width, height)) != ORBX_OK) return st;
  const OrbxPlan& P = c->plan;
  HIPCHK(c, lanes_sync(c));
  HIPCHK(c, hipMemcpy2DAsync(c->d_in, width, image, stride, width, height, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_pyramid_auto(c, c->stream, 1, c->d_in, width, (size_t)width * height));
  if (blur_enabled(c))
    HIPCHK(c, launch_blur_auto(c->blur_impl, c->stream, P, c->tm_blur, c->tiles[T_BLUR].d, c->tiles[T_BLUR].count, 1,
                               cur_lane(c).d_pyr, cur_lane(c).d_pyr_blur, c->p.blur_levels == ORBX_BLUR_UPPER ? 1 : 0,
                               c->p.blur_kind));
  const OrbxLevel& L = P.L[level];
  HIPCHK(c, hipMemcpy2DAsync(dst, L.w, final_pyr(c) + L.img_off, L.pitch, L.w, L.h, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (level_w) *level_w = L.w;
  if (level_h) *level_h = L.h;
  return ORBX_OK;
}

int orbx_select_top(orbx_ctx* c, const float* responses, int n, int keep, int32_t* indices, int* kept) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || keep < 0 || (n > 0 && (!responses || !indices)) || !kept)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad select_top arguments");
  const int m = std::min(n, keep);
  *kept = m;
  if (m == 0) return ORBX_OK;
  ENSURE(c, c->s_f32b, sizeof(float) * (size_t)n);
  ENSURE(c, c->s_i32, sizeof(int32_t) * (size_t)n);
  HIPCHK(c, hipMemcpyAsync(c->s_f32b.p, responses, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_select_flat(c->stream, (const float*)c->s_f32b.p, n, keep, (int32_t*)c->s_i32.p));
  HIPCHK(c, hipMemcpyAsync(indices, c->s_i32.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

// ---- descriptor matching (next row) -----------------------------------------

static int knn_host(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
                    double ratio, std::vector<int32_t>* idx, std::vector<int32_t>* dist,
                    std::vector<int32_t>* match) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (nq < 0 || nt < 0 || (nq > 0 && !query) || (nt > 0 && !train))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad matcher arguments");
  idx->assign((size_t)2 * nq, -1);
  dist->assign((size_t)2 * nq, -1);
  match->assign((size_t)nq, -1);
  if (nq == 0) return ORBX_OK;
  ENSURE(c, c->m_q, sizeof(orbx_descriptor) * (size_t)nq);
  ENSURE(c, c->m_t, sizeof(orbx_descriptor) * (size_t)std::max(nt, 1));
  ENSURE(c, c->m_idx, sizeof(int32_t) * 2 * (size_t)nq);
  ENSURE(c, c->m_dist, sizeof(int32_t) * 2 * (size_t)nq);
  ENSURE(c, c->m_match, sizeof(int32_t) * (size_t)nq);
  ENSURE(c, c->m_cnt, 64);
  const int32_t cnt[2] = {nq, nt};
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->m_cnt.p, cnt, sizeof(cnt), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->m_q.p, query, sizeof(orbx_descriptor) * (size_t)nq, hipMemcpyHostToDevice, s));
  if (nt > 0) HIPCHK(c, hipMemcpyAsync(c->m_t.p, train, sizeof(orbx_descriptor) * (size_t)nt, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_knn2(s, 1, nq, (const orbx_descriptor*)c->m_q.p, (const int32_t*)c->m_cnt.p, 0,
                             (const orbx_descriptor*)c->m_t.p, (const int32_t*)c->m_cnt.p + 1, 0, ratio,
                             (int32_t*)c->m_idx.p, (int32_t*)c->m_dist.p, (int32_t*)c->m_match.p, 0));
  HIPCHK(c, hipMemcpyAsync(idx->data(), c->m_idx.p, sizeof(int32_t) * 2 * (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(dist->data(), c->m_dist.p, sizeof(int32_t) * 2 * (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(match->data(), c->m_match.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->match_pairs = 0;  // the scratch no longer holds a batch's matches
  return ORBX_OK;
}

static int compact_matches(orbx_ctx* c, const int32_t* match, const int32_t* dist2, int nq, int32_t* query_idx,
                           int32_t* train_idx, int32_t* dist1, int capacity, int* count) {
  int n = 0;
  for (int i = 0; i < nq; i++)
    if (match[i] >= 0) {
      if (n < capacity) {
        query_idx[n] = i;
        train_idx[n] = match[i];
        if (dist1) dist1[n] = dist2[2 * i];
      }
      n++;
    }
  *count = n;
  return n > capacity ? fail(c, ORBX_ERR_CAPACITY, "capacity smaller than match count") : (int)ORBX_OK;
}

int orbx_knn2(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
              int32_t* idx, int32_t* dist) {
  DeviceGuard _dg(c);
  if (c && nq > 0 && (!idx || !dist)) return fail(c, ORBX_ERR_INVALID_ARG, "idx/dist is NULL");
  std::vector<int32_t> vi, vd, vm;
  int st = knn_host(c, query, nq, train, nt, 0.8, &vi, &vd, &vm);
  if (st != ORBX_OK) return st;
  if (nq > 0) {
    std::memcpy(idx, vi.data(), sizeof(int32_t) * 2 * (size_t)nq);
    std::memcpy(dist, vd.data(), sizeof(int32_t) * 2 * (size_t)nq);
  }
  return ORBX_OK;
}

int orbx_match_ratio(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
                     double ratio, int32_t* query_idx, int32_t* train_idx, int32_t* dist1, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (c && (!count || capacity < 0 || (capacity > 0 && (!query_idx || !train_idx))))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad match output arguments");
  std::vector<int32_t> vi, vd, vm;
  int st = knn_host(c, query, nq, train, nt, ratio, &vi, &vd, &vm);
  if (st != ORBX_OK) return st;
  return compact_matches(c, vm.data(), vd.data(), nq, query_idx, train_idx, dist1, capacity, count);
}

int orbx_batch_match_consecutive(orbx_ctx* c, double ratio) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const Block& B = last_block(c);
  if (B.n < 2) return fail(c, ORBX_ERR_INVALID_ARG, "needs a batch of at least two frames");
  // the match buffers are ONE set per context: a match of the other lane's batch may still be writing them
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const int n = B.n, cap = B.cap;
  const size_t e = (size_t)(n - 1) * cap;
  ENSURE(c, c->m_idx, sizeof(int32_t) * 2 * e);
  ENSURE(c, c->m_dist, sizeof(int32_t) * 2 * e);
  ENSURE(c, c->m_match, sizeof(int32_t) * e);
  const int32_t* counts = (const int32_t*)(B.d + B.layout.counts);
  const orbx_descriptor* desc = (const orbx_descriptor*)(B.d + B.layout.desc);
  hipStream_t s = batch_stream(c);
  // pair p: query = frame p, train = frame p+1 (same arrays, shifted by one slot block)
  HIPCHK(c, orbx_launch_knn2(s, n - 1, cap, desc, counts, (size_t)cap, desc + cap, counts + 1, (size_t)cap, ratio,
                             (int32_t*)c->m_idx.p, (int32_t*)c->m_dist.p, (int32_t*)c->m_match.p, (size_t)cap));
  c->match_pairs = n - 1;
  c->match_serial = c->batch_serial;
  c->match_gen++;
  return ORBX_OK;
}

int orbx_batch_match_fetch(orbx_ctx* c, int pair, int32_t* query_idx, int32_t* train_idx, int32_t* dist1,
                           int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && (!query_idx || !train_idx)))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad match output arguments");
  if (pair < 0 || pair >= c->match_pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last matched batch");
  const Block& B = last_block(c);
  const int cap = B.cap;
  hipStream_t s = batch_stream(c);
  int32_t nq = 0;
  std::vector<int32_t> vm((size_t)cap), vd((size_t)2 * cap);
  HIPCHK(c, hipMemcpyAsync(&nq, (const int32_t*)(B.d + B.layout.counts) + pair, sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(vm.data(), (const int32_t*)c->m_match.p + (size_t)pair * cap, sizeof(int32_t) * cap,
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(vd.data(), (const int32_t*)c->m_dist.p + (size_t)2 * pair * cap, sizeof(int32_t) * 2 * cap,
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return compact_matches(c, vm.data(), vd.data(), nq, query_idx, train_idx, dist1, capacity, count);
}

}  // extern "C"

// ---- pyramidal Lucas-Kanade tracking (src/feature_tracking.cpp:166-193) ------------------

namespace {
struct LkGeom {
  int top = 0;
  int w[ORBX_LK_MAX_LEVELS], h[ORBX_LK_MAX_LEVELS], pitch[ORBX_LK_MAX_LEVELS];
  size_t img_off[ORBX_LK_MAX_LEVELS], der_off[ORBX_LK_MAX_LEVELS];
  size_t img_bytes = 0, der_bytes = 0;
};
// buildOpticalFlowPyramid: halve ((w+1)/2) until a level would not be larger than the window
LkGeom lk_geometry(int w, int h, int win, int max_level) {
  LkGeom g;
  for (int l = 0; l <= max_level; l++) {
    const int lw = l == 0 ? w : (g.w[l - 1] + 1) / 2, lh = l == 0 ? h : (g.h[l - 1] + 1) / 2;
    if (l > 0 && (lw <= win || lh <= win)) break;
    g.w[l] = lw;
    g.h[l] = lh;
    g.pitch[l] = lw;  // tight: a host image with stride == width goes up in ONE contiguous copy
    g.img_off[l] = g.img_bytes;
    g.img_bytes += align_up_sz((size_t)g.pitch[l] * lh, 256);
    g.der_off[l] = g.der_bytes;
    g.der_bytes += align_up_sz((size_t)lw * lh * 4, 256);
    g.top = l;
  }
  return g;
}
OrbxLkPyr lk_pyr(const LkGeom& g, const uint8_t* img, const uint8_t* deriv) {
  OrbxLkPyr P;
  std::memset(&P, 0, sizeof(P));
  P.top = g.top;
  for (int l = 0; l <= g.top; l++) {
    P.L[l].img = img + g.img_off[l];
    P.L[l].deriv = deriv ? reinterpret_cast<const int16_t*>(deriv + g.der_off[l]) : nullptr;
    P.L[l].w = g.w[l];
    P.L[l].h = g.h[l];
    P.L[l].pitch = g.pitch[l];
  }
  return P;
}
// host image -> level 0, then pyrDown level by level
int lk_upload(orbx_ctx* c, const LkGeom& g, DevBuf& b, const uint8_t* img, int stride) {
  ENSURE(c, b, g.img_bytes + 256);
  uint8_t* base = (uint8_t*)b.p;
  if (stride == g.w[0])
    HIPCHK(c, hipMemcpyAsync(base, img, (size_t)g.w[0] * g.h[0], hipMemcpyHostToDevice, c->stream));
  else  // (row-by-row in the runtime: slow, but only for padded host images)
    HIPCHK(c, hipMemcpy2DAsync(base, g.pitch[0], img, stride, g.w[0], g.h[0], hipMemcpyHostToDevice, c->stream));
  for (int l = 1; l <= g.top; l++)
    HIPCHK(c, orbx_launch_lk_pyrdown(c->stream, base + g.img_off[l - 1], g.w[l - 1], g.h[l - 1], g.pitch[l - 1],
                                     base + g.img_off[l], g.w[l], g.h[l], g.pitch[l]));
  return ORBX_OK;
}
}  // namespace

extern "C" {

int orbx_lk_track(orbx_ctx* c, const uint8_t* prev, int prev_stride, const uint8_t* next, int next_stride, int width,
                  int height, const float* prev_pts_xy, int n, float* next_pts_xy, uint8_t* status, float* err,
                  int win_size, int max_level, int max_iters, double epsilon) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!next || n < 0 || (n > 0 && (!prev_pts_xy || !next_pts_xy || !status)))
    return fail(c, ORBX_ERR_INVALID_ARG, "next image / point arrays are NULL");
  if (width < 1 || height < 1 || next_stride < width || (prev && prev_stride < width))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad image size or stride");
  if (win_size < 3 || win_size > 31 || max_level < 0 || max_level >= ORBX_LK_MAX_LEVELS)
    return fail(c, ORBX_ERR_INVALID_ARG, "win_size must be in [3, 31], max_level in [0, 7]");
  // TermCriteria sanitising of calcOpticalFlowPyrLK
  max_iters = std::min(std::max(max_iters, 0), 100);
  epsilon = std::min(std::max(epsilon, 0.0), 10.0);
  const LkGeom g = lk_geometry(width, height, win_size, max_level);
  int st;
  int ip;  // buffer holding the `prev` pyramid
  if (prev) {
    ip = c->lk_last == 0 ? 1 : 0;
    if ((st = lk_upload(c, g, c->lk_img[ip], prev, prev_stride)) != ORBX_OK) return st;
  } else {
    // the previous call's `next` image is this call's `prev` (img1 = img2.clone(), feature_tracking.cpp:112)
    if (c->lk_last < 0 || c->lk_w != width || c->lk_h != height || c->lk_top != g.top || c->lk_win != win_size)
      return fail(c, ORBX_ERR_INVALID_ARG, "prev == NULL needs a previous orbx_lk_track call of the same geometry");
    ip = c->lk_last;
  }
  const int in = 1 - ip;
  c->lk_last = -1;  // invalid until this call has succeeded
  if ((st = lk_upload(c, g, c->lk_img[in], next, next_stride)) != ORBX_OK) return st;
  ENSURE(c, c->lk_deriv, g.der_bytes + 256);
  const uint8_t* pimg = (const uint8_t*)c->lk_img[ip].p;
  for (int l = 0; l <= g.top; l++)
    HIPCHK(c, orbx_launch_lk_scharr(c->stream, pimg + g.img_off[l], g.w[l], g.h[l], g.pitch[l],
                                    reinterpret_cast<int16_t*>((uint8_t*)c->lk_deriv.p + g.der_off[l])));
  uint8_t* hio = nullptr;
  const size_t o_out = sizeof(float) * 2 * (size_t)n, o_err = 2 * o_out, o_st = o_err + sizeof(float) * (size_t)n;
  const size_t io_bytes = o_st + (size_t)n;
  if (n > 0) {
    ENSURE(c, c->lk_io, io_bytes);
    if (c->lk_host_bytes < io_bytes) {  // pinned staging: small pageable copies cost ~15 us each
      if (c->lk_host) (void)hipHostFree(c->lk_host);
      c->lk_host = nullptr;
      c->lk_host_bytes = 0;
      HIPCHK(c, hipHostMalloc(&c->lk_host, align_up_sz(io_bytes, 4096), hipHostMallocDefault));
      c->lk_host_bytes = align_up_sz(io_bytes, 4096);
    }
    hio = (uint8_t*)c->lk_host;
    uint8_t* dio = (uint8_t*)c->lk_io.p;
    std::memcpy(hio, prev_pts_xy, o_out);
    HIPCHK(c, hipMemcpyAsync(dio, hio, o_out, hipMemcpyHostToDevice, c->stream));
    const OrbxLkPyr P = lk_pyr(g, pimg, (const uint8_t*)c->lk_deriv.p);
    const OrbxLkPyr N = lk_pyr(g, (const uint8_t*)c->lk_img[in].p, nullptr);
    HIPCHK(c, orbx_launch_lk_track(c->stream, P, N, n, (const float*)dio, (float*)(dio + o_out), dio + o_st,
                                   (float*)(dio + o_err), win_size, max_iters, epsilon * epsilon));
    HIPCHK(c, hipMemcpyAsync(hio + o_out, dio + o_out, io_bytes - o_out, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n > 0) {
    std::memcpy(next_pts_xy, hio + o_out, o_out);
    std::memcpy(status, hio + o_st, (size_t)n);
    if (err) std::memcpy(err, hio + o_err, sizeof(float) * (size_t)n);
  }
  c->lk_w = width;
  c->lk_h = height;
  c->lk_top = g.top;
  c->lk_win = win_size;
  c->lk_last = in;
  return ORBX_OK;
}

int orbx_lk_pyramid_levels(int width, int height, int win_size, int max_level) {
  if (width < 1 || height < 1 || win_size < 3 || win_size > 31 || max_level < 0 || max_level >= ORBX_LK_MAX_LEVELS)
    return -1;
  return lk_geometry(width, height, win_size, max_level).top + 1;
}

}  // extern "C"

// ---- Lucas-Kanade over frame windows ---------------------------------------------------------
// trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) for many windows per launch; with windows of two
// frames, track_optical_flow (src/feature_tracking.cpp:166-193) over a stream.

namespace {

// the workspace of ONE frame: the pyramid levels above 0 (level 0 is read in place), then the derivative maps of
// every level
struct LkwLayout {
  LkGeom g;
  size_t img_bytes, frame_bytes;  // levels 1 .. top; img_bytes + derivative maps
};
LkwLayout lkw_layout(int w, int h, int win, int max_level) {
  LkwLayout o;
  o.g = lk_geometry(w, h, win, max_level);
  o.img_bytes = o.g.top >= 1 ? o.g.img_bytes - o.g.img_off[1] : 0;
  o.frame_bytes = o.img_bytes + o.g.der_bytes;
  return o;
}

int lkw_wait(orbx_ctx* c) {
  if (c->lkw_ev) HIPCHK(c, hipEventSynchronize(c->lkw_ev));
  return ORBX_OK;
}

// a windows call on stream s: earlier windows work on another stream has to be done (one workspace, one result block)
int lkw_enter(orbx_ctx* c, hipStream_t s) {
  if (!c->lkw_ev) HIPCHK(c, hipEventCreateWithFlags(&c->lkw_ev, hipEventDisableTiming));
  if (c->lkw_stream != s) {
    const int st = lkw_wait(c);
    if (st != ORBX_OK) return st;
  }
  c->lkw_stream = s;
  return ORBX_OK;
}

struct LkwMark {
  orbx_ctx* c;
  hipStream_t s;
  ~LkwMark() {
    if (c->lkw_ev) (void)hipEventRecord(c->lkw_ev, s);
  }
};

// a buffer of the windows path of at least `bytes`: the new allocation is made BEFORE the old one is released, so
// that a failed call keeps what it had
int lkw_grow(orbx_ctx* c, DevBuf& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return ORBX_OK;
  const int st = lkw_wait(c);  // (the old allocation may still be read or written)
  if (st != ORBX_OK) return st;
  bytes = align_up_sz(std::max<size_t>(bytes, 256), 256);
  void* p = nullptr;
  HIPCHK(c, hipMalloc(&p, bytes));
  if (b.p) (void)hipFree(b.p);
  b.p = p;
  b.bytes = bytes;
  return ORBX_OK;
}

struct LkwResult {
  size_t o_seen, o_err, bytes;  // tracks at 0
};
LkwResult lkw_result(int n_windows, int cap, int len) {
  LkwResult r;
  const size_t slots = (size_t)n_windows * cap;
  r.o_seen = align_up_sz(sizeof(float) * 2 * slots * len, 256);
  r.o_err = align_up_sz(r.o_seen + sizeof(int32_t) * slots, 256);
  r.bytes = r.o_err + sizeof(float) * slots * (len - 1);
  return r;
}

// max_frames: max_batch for the device entry; the host entry stages into a buffer of its own (65535: blockIdx.z)
int lkw_check_frames(orbx_ctx* c, const void* d_frames, int n_frames, int max_frames, int width, int height,
                     int row_stride, size_t frame_stride) {
  if (!d_frames) return fail(c, ORBX_ERR_INVALID_ARG, "frames is NULL");
  if (n_frames < 2 || n_frames > max_frames)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_frames outside [2, " + std::to_string(max_frames) + "]");
  if (width < 8 || height < 8 || width > c->p.max_width || height > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "image size outside [8, max_width] x [8, max_height]");
  if (row_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "row_stride < width");
  if (frame_stride < (size_t)row_stride * (size_t)(height - 1) + (size_t)width)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame_stride smaller than a frame");
  if ((unsigned long long)row_stride * (unsigned long long)(height - 1) + (unsigned long long)width > 0x7fffffffull)
    return fail(c, ORBX_ERR_INVALID_ARG, "row_stride * (height - 1) + width exceeds 2^31 - 1");
  return ORBX_OK;
}

int lkw_check_params(orbx_ctx* c, int win_size, int max_level, int* max_iters, double* epsilon) {
  if (win_size < 3 || win_size > 31 || max_level < 0 || max_level >= ORBX_LK_MAX_LEVELS)
    return fail(c, ORBX_ERR_INVALID_ARG, "win_size must be in [3, 31], max_level in [0, 7]");
  if (!(*epsilon == *epsilon)) return fail(c, ORBX_ERR_INVALID_ARG, "epsilon is NaN");
  // TermCriteria sanitising of calcOpticalFlowPyrLK, as orbx_lk_track
  *max_iters = std::min(std::max(*max_iters, 0), 100);
  *epsilon = std::min(std::max(*epsilon, 0.0), 10.0);
  return ORBX_OK;
}

// enqueues the pyramids and the tracking of every window on s; arguments are checked
int lkw_run(orbx_ctx* c, const uint8_t* d_frames, int n_frames, int w, int h, int row_stride, size_t frame_stride,
            const int32_t* window_first, int n_windows, int window_len, const float* d_points,
            const int32_t* d_counts, int cap, int win, int max_level, int max_iters, double epsilon, hipStream_t s) {
  int st = lkw_enter(c, s);
  if (st != ORBX_OK) return st;
  const LkwMark mark{c, s};
  // points and counts may be the good-features block, written on another stream
  if (c->gf_ev && c->gf_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->gf_ev, 0));
  const LkwLayout L = lkw_layout(w, h, win, max_level);
  // frames per slice: what the limit holds, at least one window, at most the batch
  const size_t fit =
      std::min<size_t>(std::max<size_t>(c->lkw_ws_limit / L.frame_bytes, (size_t)window_len), (size_t)n_frames);
  const LkwResult R = lkw_result(n_windows, cap, window_len);
  if ((st = lkw_grow(c, c->lkw_ws, fit * L.frame_bytes + 256)) != ORBX_OK) return st;
  if ((st = lkw_grow(c, c->lkw_first, sizeof(int32_t) * (size_t)n_windows)) != ORBX_OK) return st;
  const void* old_res = c->lkw_res.p;
  if ((st = lkw_grow(c, c->lkw_res, R.bytes)) != ORBX_OK) return st;
  if (c->lkw_res.p != old_res) c->lkw_n = 0;  // (a larger block: the previous result went with the old one)
  // The window table goes up through a pinned mirror (a copy from pageable memory would make the host wait for the
  // stream).  The mirror is reused: the previous call's copy has to have read it.
  const size_t table = sizeof(int32_t) * (size_t)n_windows;
  if (!c->lkw_first_ev) HIPCHK(c, hipEventCreateWithFlags(&c->lkw_first_ev, hipEventDisableTiming));
  HIPCHK(c, hipEventSynchronize(c->lkw_first_ev));
  if (c->lkw_first_host_bytes < table) {
    if (c->lkw_first_host) (void)hipHostFree(c->lkw_first_host);
    c->lkw_first_host = nullptr;
    c->lkw_first_host_bytes = 0;
    HIPCHK(c, hipHostMalloc(&c->lkw_first_host, align_up_sz(table, 4096), hipHostMallocDefault));
    c->lkw_first_host_bytes = align_up_sz(table, 4096);
  }
  // from here on the previous result is being replaced
  c->lkw_n = 0;
  std::memcpy(c->lkw_first_host, window_first, table);
  HIPCHK(c, hipMemcpyAsync(c->lkw_first.p, c->lkw_first_host, table, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->lkw_first_ev, s));
  uint8_t* ws = (uint8_t*)c->lkw_ws.p;
  uint8_t* res = (uint8_t*)c->lkw_res.p;
  const LkGeom& g = L.g;
  const size_t img_base = g.top >= 1 ? g.img_off[1] : 0;  // workspace offsets count from level 1
  const size_t slot_stride = (size_t)cap;
  // slices of whole consecutive windows whose frames [lo, hi) fit the workspace
  for (int w0 = 0; w0 < n_windows;) {
    int lo = window_first[w0], hi = lo + window_len, w1 = w0 + 1;
    while (w1 < n_windows && w1 - w0 < 65535) {
      const int nlo = std::min(lo, window_first[w1]), nhi = std::max(hi, window_first[w1] + window_len);
      if ((size_t)(nhi - nlo) > fit) break;
      lo = nlo;
      hi = nhi;
      w1++;
    }
    const int m = hi - lo;
    uint8_t* ws_img = ws;                                // [m][levels 1 .. top]
    uint8_t* ws_der = ws + align_up_sz(L.img_bytes * m, 256);  // [m][levels 0 .. top]
    const uint8_t* f_lo = d_frames + frame_stride * (size_t)lo;
    for (int l = 1; l <= g.top; l++) {
      const uint8_t* src = l == 1 ? f_lo : ws_img + (g.img_off[l - 1] - img_base);
      HIPCHK(c, orbx_launch_lk_pyrdown_frames(s, m, src, g.w[l - 1], g.h[l - 1], l == 1 ? row_stride : g.pitch[l - 1],
                                              l == 1 ? frame_stride : L.img_bytes, ws_img + (g.img_off[l] - img_base),
                                              g.w[l], g.h[l], g.pitch[l], L.img_bytes));
    }
    for (int l = 0; l <= g.top; l++)
      HIPCHK(c, orbx_launch_lk_scharr_frames(s, m, l == 0 ? f_lo : ws_img + (g.img_off[l] - img_base), g.w[l], g.h[l],
                                             l == 0 ? row_stride : g.pitch[l], l == 0 ? frame_stride : L.img_bytes,
                                             reinterpret_cast<int16_t*>(ws_der + g.der_off[l]), g.der_bytes));
    OrbxLkFrames F;
    std::memset(&F, 0, sizeof(F));
    F.top = g.top;
    F.first = lo;
    F.frame_stride = frame_stride;
    F.img_stride = L.img_bytes;
    F.der_stride = g.der_bytes / sizeof(int16_t);
    for (int l = 0; l <= g.top; l++) {
      F.L[l].img = l == 0 ? d_frames : ws_img + (g.img_off[l] - img_base);
      F.L[l].deriv = reinterpret_cast<const int16_t*>(ws_der + g.der_off[l]);
      F.L[l].w = g.w[l];
      F.L[l].h = g.h[l];
      F.L[l].pitch = l == 0 ? row_stride : g.pitch[l];
    }
    HIPCHK(c, orbx_launch_lk_track_windows(
                  s, F, (const int32_t*)c->lkw_first.p + w0, w1 - w0, window_len, d_points + 2 * slot_stride * w0,
                  d_counts ? d_counts + w0 : nullptr, cap, (float*)res + 2 * slot_stride * window_len * w0,
                  (int32_t*)(res + R.o_seen) + slot_stride * w0,
                  (float*)(res + R.o_err) + slot_stride * (window_len - 1) * w0, win, max_iters, epsilon * epsilon));
    w0 = w1;
  }
  c->lkw_n = n_windows;
  c->lkw_cap = cap;
  c->lkw_len = window_len;
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_lk_track_windows_device(orbx_ctx* c, const void* d_frames, int n_frames, int width, int height,
                                 int row_stride, size_t frame_stride, const int32_t* window_first, int n_windows,
                                 int window_len, const float* d_points_xy, const int32_t* d_counts, int slot_capacity,
                                 int win_size, int max_level, int max_iters, double epsilon, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = lkw_check_frames(c, d_frames, n_frames, c->p.max_batch, width, height, row_stride, frame_stride);
  if (st != ORBX_OK) return st;
  if ((st = lkw_check_params(c, win_size, max_level, &max_iters, &epsilon)) != ORBX_OK) return st;
  if (!window_first || !d_points_xy) return fail(c, ORBX_ERR_INVALID_ARG, "window_first / d_points_xy is NULL");
  if (n_windows < 1 || window_len < 2 || slot_capacity < 1)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1, window_len < 2 or slot_capacity < 1");
  for (int i = 0; i < n_windows; i++)
    if (window_first[i] < 0 || window_first[i] > n_frames - window_len)
      return fail(c, ORBX_ERR_INVALID_ARG, "a window does not lie inside the frames");
  return lkw_run(c, (const uint8_t*)d_frames, n_frames, width, height, row_stride, frame_stride, window_first,
                 n_windows, window_len, d_points_xy, d_counts, slot_capacity, win_size, max_level, max_iters, epsilon,
                 stream ? (hipStream_t)stream : c->stream);
}

int orbx_lk_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = lkw_wait(c);
  if (st != ORBX_OK) return st;
  if (c->lkw_ws.p) {
    HIPCHK(c, hipFree(c->lkw_ws.p));
    c->lkw_ws = DevBuf{};
  }
  c->lkw_ws_limit = bytes ? bytes : ORBX_LK_WORKSPACE_DEFAULT;
  return ORBX_OK;
}

int orbx_lk_windows_results_device(orbx_ctx* c, orbx_lk_windows_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->lkw_n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  const LkwResult R = lkw_result(c->lkw_n, c->lkw_cap, c->lkw_len);
  const uint8_t* res = (const uint8_t*)c->lkw_res.p;
  v->tracks_xy = (const float*)res;
  v->seen = (const int32_t*)(res + R.o_seen);
  v->err = (const float*)(res + R.o_err);
  v->slot_capacity = c->lkw_cap;
  v->window_len = c->lkw_len;
  v->n_windows = c->lkw_n;
  return ORBX_OK;
}

int orbx_lk_windows_fetch(orbx_ctx* c, int first, int n, float* tracks_xy, int32_t* seen, float* err) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->lkw_n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  if (first < 0 || n < 1 || first >= c->lkw_n || n > c->lkw_n - first)
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the batch");
  const int st = lkw_wait(c);
  if (st != ORBX_OK) return st;
  const LkwResult R = lkw_result(c->lkw_n, c->lkw_cap, c->lkw_len);
  const uint8_t* res = (const uint8_t*)c->lkw_res.p;
  const size_t slots = (size_t)c->lkw_cap, len = (size_t)c->lkw_len;
  if (tracks_xy)
    HIPCHK(c, hipMemcpy(tracks_xy, res + sizeof(float) * 2 * slots * len * first, sizeof(float) * 2 * slots * len * n,
                        hipMemcpyDeviceToHost));
  if (seen)
    HIPCHK(c, hipMemcpy(seen, res + R.o_seen + sizeof(int32_t) * slots * first, sizeof(int32_t) * slots * n,
                        hipMemcpyDeviceToHost));
  if (err)
    HIPCHK(c, hipMemcpy(err, res + R.o_err + sizeof(float) * slots * (len - 1) * first,
                        sizeof(float) * slots * (len - 1) * n, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_lk_track_window(orbx_ctx* c, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                         size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen, float* err,
                         int win_size, int max_level, int max_iters, double epsilon) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = lkw_check_frames(c, frames, n_frames, 65535, width, height, row_stride, frame_stride);
  if (st != ORBX_OK) return st;
  if ((st = lkw_check_params(c, win_size, max_level, &max_iters, &epsilon)) != ORBX_OK) return st;
  if (n < 0 || (n > 0 && (!pts_xy || !tracks_xy || !seen)))
    return fail(c, ORBX_ERR_INVALID_ARG, "n < 0 or pts_xy / tracks_xy / seen is NULL");
  if (n == 0) return ORBX_OK;  // no points: nothing to track, the last result stays
  if ((st = lkw_enter(c, c->stream)) != ORBX_OK) return st;
  const size_t tight = (size_t)width * height;
  {
    const LkwMark mark{c, c->stream};
    if ((st = lkw_grow(c, c->lkw_img, tight * n_frames)) != ORBX_OK) return st;
    if ((st = lkw_grow(c, c->lkw_pts, sizeof(float) * 2 * (size_t)n)) != ORBX_OK) return st;
    if (row_stride == width && frame_stride == tight) {
      HIPCHK(c, hipMemcpyAsync(c->lkw_img.p, frames, tight * n_frames, hipMemcpyHostToDevice, c->stream));
    } else {
      for (int i = 0; i < n_frames; i++)
        HIPCHK(c, hipMemcpy2DAsync((uint8_t*)c->lkw_img.p + tight * i, width, frames + frame_stride * i, row_stride,
                                   width, height, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->lkw_pts.p, pts_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  const int32_t first = 0;
  if ((st = lkw_run(c, (const uint8_t*)c->lkw_img.p, n_frames, width, height, width, tight, &first, 1, n_frames,
                    (const float*)c->lkw_pts.p, nullptr, n, win_size, max_level, max_iters, epsilon, c->stream)) !=
      ORBX_OK)
    return st;
  return orbx_lk_windows_fetch(c, 0, 1, tracks_xy, seen, err);
}

}  // extern "C"

// ---- relative pose (next row) ---------------------------

namespace {
bool pose_args_ok(const double* K, double prob, double threshold, int max_iters) {
  return K && K[0] > 0 && K[4] > 0 && std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) &&
         std::isfinite(K[5]) && std::isfinite(prob) && std::isfinite(threshold) && threshold >= 0 && max_iters >= 0;
}
void pose_unpack(const OrbxPoseOut& r, double* E, double* R, double* t, int32_t* inliers, int32_t* good,
                 int32_t* iters) {
  if (E) memcpy(E, r.E, sizeof r.E);
  if (R) memcpy(R, r.R, sizeof r.R);
  if (t) memcpy(t, r.t, sizeof r.t);
  if (inliers) *inliers = r.inliers;
  if (good) *good = r.good;
  if (iters) *iters = r.iters;
}
}  // namespace

extern "C" {

int orbx_estimate_pose(orbx_ctx* c, const float* pts1_xy, const float* pts2_xy, int n, const double* K, double prob,
                       double threshold, int max_iters, uint64_t seed, double* E, double* R, double* t, uint8_t* mask,
                       int32_t* inliers, int32_t* good, int32_t* iters) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!pts1_xy || !pts2_xy)) || !E || !R || !t || !inliers || !good || !iters ||
      !pose_args_ok(K, prob, threshold, max_iters))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  const int cap = n > 0 ? n : 1;
  ENSURE(c, c->ph_in, sizeof(float) * 4 * (size_t)cap);
  ENSURE(c, c->ph_pts, sizeof(OrbxPosePt) * (size_t)cap);
  ENSURE(c, c->ph_n, sizeof(int32_t));
  ENSURE(c, c->ph_out, sizeof(OrbxPoseOut));
  ENSURE(c, c->ph_mask, (size_t)cap);
  hipStream_t s = c->stream;
  float* d_p1 = (float*)c->ph_in.p;
  float* d_p2 = d_p1 + 2 * (size_t)cap;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(d_p1, pts1_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_p2, pts2_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, orbx_launch_pose_prep_host(s, n, d_p1, d_p2, K, (OrbxPosePt*)c->ph_pts.p, (int32_t*)c->ph_n.p));
  HIPCHK(c, orbx_launch_pose_ransac(s, 1, cap, (const OrbxPosePt*)c->ph_pts.p, (const int32_t*)c->ph_n.p, K, prob,
                                    threshold, max_iters, seed, (OrbxPoseOut*)c->ph_out.p, (uint8_t*)c->ph_mask.p));
  OrbxPoseOut r;
  HIPCHK(c, hipMemcpyAsync(&r, c->ph_out.p, sizeof r, hipMemcpyDeviceToHost, s));
  if (mask && n > 0) HIPCHK(c, hipMemcpyAsync(mask, c->ph_mask.p, (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  pose_unpack(r, E, R, t, inliers, good, iters);
  return ORBX_OK;
}

int orbx_batch_pose_consecutive(orbx_ctx* c, const double* K, double prob, double threshold, int max_iters,
                                uint64_t seed) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!pose_args_ok(K, prob, threshold, max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if (c->match_pairs <= 0 || c->match_serial != c->batch_serial)
    return fail(c, ORBX_ERR_INVALID_ARG, "the last batch has not been matched (orbx_batch_match_consecutive)");
  // the pose buffers are ONE set per context, like the matcher's
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const Block& B = last_block(c);
  const int npairs = c->match_pairs, cap = B.cap;
  const size_t e = (size_t)npairs * cap;
  ENSURE(c, c->pb_pts, sizeof(OrbxPosePt) * e);
  ENSURE(c, c->pb_n, sizeof(int32_t) * (size_t)npairs);
  ENSURE(c, c->pb_out, sizeof(OrbxPoseOut) * (size_t)npairs);
  ENSURE(c, c->pb_mask, e);
  const OutLayout& o = B.layout;
  hipStream_t s = batch_stream(c);
  HIPCHK(c, orbx_launch_pose_prep_batch(s, npairs, cap, (const int32_t*)(B.d + o.counts),
                                        (const orbx_keypoint*)(B.d + o.kp), (const int32_t*)c->m_match.p, K,
                                        (OrbxPosePt*)c->pb_pts.p, (int32_t*)c->pb_n.p));
  HIPCHK(c, orbx_launch_pose_ransac(s, npairs, cap, (const OrbxPosePt*)c->pb_pts.p, (const int32_t*)c->pb_n.p, K, prob,
                                    threshold, max_iters, seed, (OrbxPoseOut*)c->pb_out.p, (uint8_t*)c->pb_mask.p));
  c->pose_pairs = npairs;
  c->pose_cap = cap;
  c->pose_stream = s;
  c->pose_serial = c->batch_serial;
  c->pose_match_gen = c->match_gen;
  return ORBX_OK;
}

int orbx_batch_pose_fetch(orbx_ctx* c, int first, int n, double* E, double* R, double* t, int32_t* inliers,
                          int32_t* good, int32_t* iters) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->pose_pairs <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been posed");
  if (first < 0 || n < 0 || first + n > c->pose_pairs)
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last posed batch");
  if (n == 0) return ORBX_OK;
  std::vector<OrbxPoseOut> r((size_t)n);
  HIPCHK(c, hipMemcpyAsync(r.data(), (const OrbxPoseOut*)c->pb_out.p + first, sizeof(OrbxPoseOut) * (size_t)n,
                           hipMemcpyDeviceToHost, c->pose_stream));
  HIPCHK(c, hipStreamSynchronize(c->pose_stream));
  for (int i = 0; i < n; i++)
    pose_unpack(r[(size_t)i], E ? E + 9 * i : nullptr, R ? R + 9 * i : nullptr, t ? t + 3 * i : nullptr,
                inliers ? inliers + i : nullptr, good ? good + i : nullptr, iters ? iters + i : nullptr);
  return ORBX_OK;
}

int orbx_batch_pose_mask(orbx_ctx* c, int pair, uint8_t* mask, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && !mask)) return fail(c, ORBX_ERR_INVALID_ARG, "bad mask arguments");
  if (pair < 0 || pair >= c->pose_pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last posed batch");
  int32_t np = 0;
  HIPCHK(c, hipMemcpyAsync(&np, (const int32_t*)c->pb_n.p + pair, sizeof np, hipMemcpyDeviceToHost, c->pose_stream));
  HIPCHK(c, hipStreamSynchronize(c->pose_stream));
  *count = np;
  if (np > capacity) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than the pair's match count");
  if (np > 0) {
    HIPCHK(c, hipMemcpyAsync(mask, (const uint8_t*)c->pb_mask.p + (size_t)pair * c->pose_cap, (size_t)np,
                             hipMemcpyDeviceToHost, c->pose_stream));
    HIPCHK(c, hipStreamSynchronize(c->pose_stream));
  }
  return ORBX_OK;
}

}  // extern "C"

// ---- triangulation, relative scale, trajectory chaining ------------

namespace {
bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}
}  // namespace

extern "C" {

int orbx_triangulate(orbx_ctx* c, const float* pts1_xy, const float* pts2_xy, int n, const double* K, const double* R,
                     const double* t, float* xyz, uint8_t* valid) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!pts1_xy || !pts2_xy || !xyz || !valid)) || !K || !R || !t || !finite_all(K, 9) ||
      !finite_all(R, 9) || !finite_all(t, 3))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad triangulation arguments");
  if (n == 0) return ORBX_OK;
  ENSURE(c, c->sh_in, sizeof(float) * 4 * (size_t)n);
  ENSURE(c, c->sh_xyz, sizeof(float) * 3 * (size_t)n);
  ENSURE(c, c->sh_valid, (size_t)n);
  hipStream_t s = c->stream;
  float* d_p1 = (float*)c->sh_in.p;
  float* d_p2 = d_p1 + 2 * (size_t)n;
  HIPCHK(c, hipMemcpyAsync(d_p1, pts1_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_p2, pts2_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_triangulate_host(s, n, d_p1, d_p2, K, R, t, (float*)c->sh_xyz.p, (uint8_t*)c->sh_valid.p));
  HIPCHK(c, hipMemcpyAsync(xyz, c->sh_xyz.p, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(valid, c->sh_valid.p, (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return ORBX_OK;
}

int orbx_estimate_scale(orbx_ctx* c, const float* prev_xyz, const uint8_t* prev_valid, int n_prev, const float* cur_xyz,
                        const uint8_t* cur_valid, int n_cur, double* scale, int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n_prev < 0 || n_cur < 0 || (n_prev > 0 && !prev_xyz) || (n_cur > 0 && !cur_xyz) || !scale || !ratios_used)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad scale arguments");
  const int m = std::min(n_prev, n_cur);
  if (m == 0) {  // src/feature_matching.cpp:248-249
    *scale = 1.0;
    *ratios_used = 0;
    return ORBX_OK;
  }
  if ((size_t)m * 8 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more aligned points than the selection holds in LDS");
  // only the first m points of either list enter
  ENSURE(c, c->sh_xyz, sizeof(float) * 6 * (size_t)m);
  ENSURE(c, c->sh_valid, 2 * (size_t)m);
  ENSURE(c, c->sh_out, sizeof(OrbxScaleOut));
  hipStream_t s = c->stream;
  float* d_prev = (float*)c->sh_xyz.p;
  float* d_cur = d_prev + 3 * (size_t)m;
  uint8_t* d_pv = (uint8_t*)c->sh_valid.p;
  uint8_t* d_cv = d_pv + m;
  HIPCHK(c, hipMemcpyAsync(d_prev, prev_xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_cur, cur_xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
  if (prev_valid) HIPCHK(c, hipMemcpyAsync(d_pv, prev_valid, (size_t)m, hipMemcpyHostToDevice, s));
  if (cur_valid) HIPCHK(c, hipMemcpyAsync(d_cv, cur_valid, (size_t)m, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_scale_aligned(s, m, m, d_prev, prev_valid ? d_pv : nullptr, d_cur, cur_valid ? d_cv : nullptr,
                                      (OrbxScaleOut*)c->sh_out.p));
  OrbxScaleOut r;
  HIPCHK(c, hipMemcpyAsync(&r, c->sh_out.p, sizeof r, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  *scale = r.scale;
  *ratios_used = r.ratios_used;
  return ORBX_OK;
}

int orbx_batch_scale_consecutive(orbx_ctx* c, const double* K) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!K || !finite_all(K, 9)) return fail(c, ORBX_ERR_INVALID_ARG, "bad scale arguments");
  if (c->pose_pairs <= 0 || c->pose_serial != c->batch_serial)
    return fail(c, ORBX_ERR_INVALID_ARG, "the last batch has not been posed (orbx_batch_pose_consecutive)");
  // the triangulation reads the match table again: it must still hold the matches the poses were computed from
  // (a host-array matcher call reuses the scratch and zeroes match_pairs; a second batch match bumps match_gen)
  if (c->match_pairs != c->pose_pairs || c->match_serial != c->batch_serial || c->pose_match_gen != c->match_gen)
    return fail(c, ORBX_ERR_INVALID_ARG, "the match table has been rewritten since the batch was posed");
  const int npairs = c->pose_pairs, cap = c->pose_cap;
  if ((size_t)cap * 16 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more result slots per frame than the join holds in LDS");
  // the scale buffers are ONE set per context, like the pose buffers
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const size_t e = (size_t)npairs * cap;
  ENSURE(c, c->sb_xyz, sizeof(float) * 3 * e);
  ENSURE(c, c->sb_valid, e);
  ENSURE(c, c->sb_mq, sizeof(int32_t) * e);
  ENSURE(c, c->sb_mt, sizeof(int32_t) * e);
  ENSURE(c, c->sb_n, sizeof(int32_t) * (size_t)npairs);
  ENSURE(c, c->sb_out, sizeof(OrbxScaleOut) * (size_t)npairs);
  const Block& B = last_block(c);
  const OutLayout& o = B.layout;
  hipStream_t s = c->pose_stream;
  HIPCHK(c, orbx_launch_triangulate_batch(s, npairs, cap, (const int32_t*)(B.d + o.counts),
                                          (const orbx_keypoint*)(B.d + o.kp), (const int32_t*)c->m_match.p,
                                          (const OrbxPoseOut*)c->pb_out.p, K, (float*)c->sb_xyz.p,
                                          (uint8_t*)c->sb_valid.p, (int32_t*)c->sb_mq.p, (int32_t*)c->sb_mt.p,
                                          (int32_t*)c->sb_n.p));
  HIPCHK(c, orbx_launch_scale_join(s, npairs, cap, (const int32_t*)c->sb_n.p, (const int32_t*)c->sb_mq.p,
                                   (const int32_t*)c->sb_mt.p, (const float*)c->sb_xyz.p,
                                   (const uint8_t*)c->sb_valid.p, (const OrbxPoseOut*)c->pb_out.p,
                                   (OrbxScaleOut*)c->sb_out.p));
  c->scale_pairs = npairs;
  c->scale_cap = cap;
  c->scale_stream = s;
  return ORBX_OK;
}

int orbx_batch_scale_fetch(orbx_ctx* c, int first, int n, double* scale, int32_t* triplets, int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->scale_pairs <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been scaled");
  if (first < 0 || n < 0 || first + n > c->scale_pairs)
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last scaled batch");
  if (n == 0) return ORBX_OK;
  std::vector<OrbxScaleOut> r((size_t)n);
  HIPCHK(c, hipMemcpyAsync(r.data(), (const OrbxScaleOut*)c->sb_out.p + first, sizeof(OrbxScaleOut) * (size_t)n,
                           hipMemcpyDeviceToHost, c->scale_stream));
  HIPCHK(c, hipStreamSynchronize(c->scale_stream));
  for (int i = 0; i < n; i++) {
    if (scale) scale[i] = r[(size_t)i].scale;
    if (triplets) triplets[i] = r[(size_t)i].triplets;
    if (ratios_used) ratios_used[i] = r[(size_t)i].ratios_used;
  }
  return ORBX_OK;
}

int orbx_batch_points_fetch(orbx_ctx* c, int pair, float* xyz, uint8_t* valid, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && (!xyz || !valid)))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad point output arguments");
  if (pair < 0 || pair >= c->scale_pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last scaled batch");
  hipStream_t s = c->scale_stream;
  int32_t np = 0;
  HIPCHK(c, hipMemcpyAsync(&np, (const int32_t*)c->sb_n.p + pair, sizeof np, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  *count = np;
  if (np > capacity) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than the pair's match count");
  if (np > 0) {
    const size_t row = (size_t)pair * c->scale_cap;
    HIPCHK(c, hipMemcpyAsync(xyz, (const float*)c->sb_xyz.p + 3 * row, sizeof(float) * 3 * (size_t)np,
                             hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(valid, (const uint8_t*)c->sb_valid.p + row, (size_t)np, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return ORBX_OK;
}

int orbx_chain_trajectory(const double* T0, const double* R, const double* t, const double* scale, int n,
                          double* poses) {
  if (!T0 || !poses || n < 0 || (n > 0 && (!R || !t || !scale))) return ORBX_ERR_INVALID_ARG;
  std::memcpy(poses, T0, sizeof(double) * 16);
  for (int i = 0; i < n; i++) tri_chain(poses + 16 * i, R + 9 * i, t + 3 * i, scale[i], poses + 16 * (i + 1));
  return ORBX_OK;
}

}  // extern "C"

// ---- bundle adjustment -----------------------------------------------

static_assert(sizeof(orbx_ba_summary) == 32, "orbx_ba_summary is the kernel's BaSummary");

extern "C" {

int orbx_bundle_adjust_batch(orbx_ctx* c, const double* K, int n_windows, const int32_t* pose_offset, double* poses6,
                             const int32_t* point_offset, double* points3, const int32_t* obs_offset,
                             const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             double huber_delta, int max_iters, orbx_ba_summary* summaries) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!K || !finite_all(K, 9) || n_windows < 0 || !(huber_delta > 0.0) || !std::isfinite(huber_delta) ||
      max_iters < 1 || max_iters > 1000)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  if (n_windows == 0) return ORBX_OK;
  if (!pose_offset || !poses6 || !point_offset || !points3 || !obs_offset || !obs_point || !obs_pose || !obs_xy ||
      !summaries)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  if (pose_offset[0] != 0 || point_offset[0] != 0 || obs_offset[0] != 0)
    return fail(c, ORBX_ERR_INVALID_ARG, "offset arrays start at 0");
  int cap = 1, ocap = 1;
  for (int w = 0; w < n_windows; w++) {
    const long long W = (long long)pose_offset[w + 1] - pose_offset[w], N = (long long)point_offset[w + 1] - point_offset[w],
                    M = (long long)obs_offset[w + 1] - obs_offset[w];
    if (W < 2 || W > ORBX_BA_MAX_POSES) return fail(c, ORBX_ERR_INVALID_ARG, "a window has 2 .. 8 poses");
    if (N < 1 || M < N || M > N * W)
      return fail(c, ORBX_ERR_INVALID_ARG, "every landmark has 1 .. n_poses observations");
    if (N > ORBX_BA_MAX_POINTS) return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks in a window than 65536");
    cap = std::max(cap, (int)N);
    ocap = std::max(ocap, (int)M);
  }
  const size_t tp = (size_t)pose_offset[n_windows], tn = (size_t)point_offset[n_windows], tm = (size_t)obs_offset[n_windows];
  if (tn + (size_t)n_windows > 0x7fffffffu || tm > 0x7fffffffu)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks or observations in a batch than 32-bit offsets hold");
  if (!finite_all(poses6, (int)(6 * tp))) return fail(c, ORBX_ERR_INVALID_ARG, "a pose is not finite");
  for (size_t i = 0; i < 3 * tn; i++)
    if (!std::isfinite(points3[i])) return fail(c, ORBX_ERR_INVALID_ARG, "a point is not finite");
  for (size_t i = 0; i < 2 * tm; i++)
    if (!std::isfinite(obs_xy[i])) return fail(c, ORBX_ERR_INVALID_ARG, "an observation is not finite");
  // CSR by (landmark, pose), per window (src/with_bundle_adjustment.cpp:651-666 adds the residual blocks landmark by
  // landmark)
  std::vector<int32_t> rows(tn + (size_t)n_windows), order;
  std::vector<uint8_t> opose(tm);
  std::vector<double> oxy(2 * tm);
  for (int w = 0; w < n_windows; w++) {
    const int W = pose_offset[w + 1] - pose_offset[w], N = point_offset[w + 1] - point_offset[w];
    const int M = obs_offset[w + 1] - obs_offset[w];
    const int32_t* op = obs_point + obs_offset[w];
    const int32_t* oq = obs_pose + obs_offset[w];
    for (int k = 0; k < M; k++)
      if (op[k] < 0 || op[k] >= N || oq[k] < 0 || oq[k] >= W)
        return fail(c, ORBX_ERR_INVALID_ARG, "an observation's landmark or pose index is out of range");
    // every (landmark, pose) occurs at most once, so placing observation k at key landmark * W + pose and reading
    // the keys in ascending order IS the stable sort by (landmark, pose)
    order.assign((size_t)N * W, -1);
    for (int k = 0; k < M; k++) {
      int32_t& at = order[(size_t)op[k] * W + oq[k]];
      if (at >= 0) return fail(c, ORBX_ERR_INVALID_ARG, "a landmark is observed twice by one pose");
      at = k;
    }
    int32_t* row = rows.data() + point_offset[w] + w;
    std::fill(row, row + N + 1, 0);
    size_t dst = (size_t)obs_offset[w];
    for (size_t key = 0; key < order.size(); key++) {
      const int o = order[key];
      if (o < 0) continue;
      row[op[o] + 1]++;
      opose[dst] = (uint8_t)oq[o];
      oxy[2 * dst] = obs_xy[2 * ((size_t)obs_offset[w] + o)];
      oxy[2 * dst + 1] = obs_xy[2 * ((size_t)obs_offset[w] + o) + 1];
      dst++;
    }
    for (int j = 0; j < N; j++) {
      if (row[j + 1] == 0) return fail(c, ORBX_ERR_INVALID_ARG, "a landmark has no observation");
      row[j + 1] += row[j];
    }
  }
  // workgroups: as many as windows, bounded by ORBX_BA_MAX_GROUPS and by the workspace budget
  const size_t per_group = sizeof(double) * ((size_t)ORBX_BA_WS_POINT * cap + (size_t)ORBX_BA_WS_OBS * ocap) + 8 * (size_t)cap;
  int groups = std::min(n_windows, ORBX_BA_MAX_GROUPS);
  groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, ORBX_BA_WS_BUDGET / per_group));
  const size_t noff = (size_t)n_windows + 1;
  ENSURE(c, c->ba_off, sizeof(int32_t) * 3 * noff);
  ENSURE(c, c->ba_poses, sizeof(double) * 6 * tp);
  ENSURE(c, c->ba_points, sizeof(double) * 3 * tn);
  ENSURE(c, c->ba_rows, sizeof(int32_t) * rows.size());
  ENSURE(c, c->ba_opose, tm);
  ENSURE(c, c->ba_oxy, sizeof(double) * 2 * tm);
  ENSURE(c, c->ba_wp, sizeof(double) * ORBX_BA_WS_POINT * (size_t)cap * groups);
  ENSURE(c, c->ba_wo, sizeof(double) * ORBX_BA_WS_OBS * (size_t)ocap * groups);
  ENSURE(c, c->ba_slot, 8 * (size_t)cap * groups);
  ENSURE(c, c->ba_out, sizeof(orbx_ba_summary) * (size_t)n_windows);
  hipStream_t s = c->stream;
  int32_t* d_off = (int32_t*)c->ba_off.p;
  HIPCHK(c, hipMemcpyAsync(d_off, pose_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_off + noff, point_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_off + 2 * noff, obs_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ba_poses.p, poses6, sizeof(double) * 6 * tp, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ba_points.p, points3, sizeof(double) * 3 * tn, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ba_rows.p, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ba_opose.p, opose.data(), tm, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ba_oxy.p, oxy.data(), sizeof(double) * 2 * tm, hipMemcpyHostToDevice, s));
  const double K4[4] = {K[0], K[4], K[2], K[5]};
  HIPCHK(c, orbx_launch_ba(s, n_windows, groups, max_iters, K4, huber_delta, d_off, d_off + noff, d_off + 2 * noff,
                           (double*)c->ba_poses.p, (double*)c->ba_points.p, (const int32_t*)c->ba_rows.p,
                           (const uint8_t*)c->ba_opose.p, (const double*)c->ba_oxy.p, cap, ocap, (double*)c->ba_wp.p,
                           (double*)c->ba_wo.p, (unsigned long long*)c->ba_slot.p, c->ba_out.p));
  // the staged vectors are pageable: their copies above have left the host before the calls returned
  HIPCHK(c, hipMemcpyAsync(poses6, c->ba_poses.p, sizeof(double) * 6 * tp, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(points3, c->ba_points.p, sizeof(double) * 3 * tn, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(summaries, c->ba_out.p, sizeof(orbx_ba_summary) * (size_t)n_windows, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return ORBX_OK;
}

int orbx_bundle_adjust(orbx_ctx* c, const double* K, int n_poses, double* poses6, int n_points, double* points3,
                       int n_obs, const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                       double huber_delta, int max_iters, orbx_ba_summary* summary) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n_poses < 0 || n_points < 0 || n_obs < 0) return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  const int32_t po[2] = {0, n_poses}, pt[2] = {0, n_points}, ob[2] = {0, n_obs};
  return orbx_bundle_adjust_batch(c, K, 1, po, poses6, pt, points3, ob, obs_point, obs_pose, obs_xy, huber_delta,
                                  max_iters, summary);
}

}  // extern "C"

// ---- Shi-Tomasi corners (next row) ------------------------
namespace {

// the sections of the workspace for m frames of w x h with a cell grid of grid_stride words per frame
struct GfLayout {
  size_t map, keys, grid, cnt, total, pool, grid_stride;
};
GfLayout gf_layout(int m, int w, int h, size_t grid_stride) {
  GfLayout o;
  const size_t px = (size_t)w * h;
  o.pool = (size_t)(w - 2) * (h - 2);
  o.grid_stride = grid_stride;
  o.map = 0;
  o.keys = align_up_sz(sizeof(float) * px * m, 256);
  o.grid = align_up_sz(o.keys + sizeof(unsigned long long) * o.pool * m, 256);
  o.cnt = align_up_sz(o.grid + sizeof(uint32_t) * grid_stride * m, 256);
  o.total = o.cnt + 2 * sizeof(uint32_t) * (size_t)m;  // maxima, then candidate counts
  return o;
}
// the largest grid of a w x h frame: w * h cells of one slot (cell 1) or, from cell 2 on, at most
// ceil(w / 2) * ceil(h / 2) cells of four -- both within (w + 1)(h + 1) words
size_t gf_grid_bound(int w, int h) { return (size_t)(w + 1) * (h + 1); }

struct GfArgs {
  int cap, suppress, cell, gw, gh, slots;
  double quality, min_distance;
};

int gf_check_params(orbx_ctx* c, double quality, double min_distance) {
  if (!std::isfinite(quality) || !(quality > 0.0) || quality > 1.0)
    return fail(c, ORBX_ERR_INVALID_ARG, "quality_level must be finite, in (0, 1]");
  if (!std::isfinite(min_distance) || min_distance < 0.0)
    return fail(c, ORBX_ERR_INVALID_ARG, "min_distance must be finite, >= 0");
  if (min_distance > ORBX_GFTT_MAX_MIN_DISTANCE)
    return fail(c, ORBX_ERR_UNSUPPORTED, "min_distance above ORBX_GFTT_MAX_MIN_DISTANCE");
  return ORBX_OK;
}

GfArgs gf_args(int w, int h, int max_corners, double quality, double min_distance) {
  GfArgs a;
  const long long pool = (long long)(w - 2) * (h - 2);
  a.cap = (int)(max_corners > 0 ? std::min<long long>(max_corners, pool) : pool);
  a.quality = quality;
  a.min_distance = min_distance;
  a.suppress = min_distance >= 1.0;
  a.cell = a.suppress ? (int)std::nearbyint(min_distance) : 1;  // cvRound: half to even (default rounding mode)
  a.gw = (w + a.cell - 1) / a.cell;
  a.gh = (h + a.cell - 1) / a.cell;
  a.slots = a.cell == 1 ? 1 : 4;
  return a;
}

// waits for the good-features work enqueued so far, on whatever stream it ran: through the event recorded behind it,
// never through the stream itself (a caller's stream need not outlive its batch's end)
int gf_wait(orbx_ctx* c) {
  if (c->gf_ev) HIPCHK(c, hipEventSynchronize(c->gf_ev));
  return ORBX_OK;
}

// a good-features call on stream s: earlier good-features work on another stream has to be done (one workspace)
int gf_enter(orbx_ctx* c, hipStream_t s) {
  if (!c->gf_ev) HIPCHK(c, hipEventCreateWithFlags(&c->gf_ev, hipEventDisableTiming));
  if (c->gf_stream != s) {
    const int st = gf_wait(c);
    if (st != ORBX_OK) return st;
  }
  c->gf_stream = s;
  return ORBX_OK;
}

// records the event behind whatever a good-features call has enqueued on s, on every way out of the call
struct GfMark {
  orbx_ctx* c;
  hipStream_t s;
  ~GfMark() {
    if (c->gf_ev) (void)hipEventRecord(c->gf_ev, s);
  }
};

// the workspace: allocated once, for as many frames of the largest size as the limit holds (at least one, at most
// max_batch)
int gf_workspace(orbx_ctx* c) {
  if (c->gf_ws.p) return ORBX_OK;
  const int mw = c->p.max_width, mh = c->p.max_height;
  const size_t one = gf_layout(1, mw, mh, gf_grid_bound(mw, mh)).total + 1024;
  const size_t frames = std::min<size_t>(std::max<size_t>(c->gf_ws_limit / one, 1), (size_t)c->p.max_batch);
  ENSURE(c, c->gf_ws, gf_layout((int)frames, mw, mh, gf_grid_bound(mw, mh)).total + 1024);
  return ORBX_OK;
}

// frames of w x h per slice
int gf_slice_frames(const orbx_ctx* c, int n, int w, int h, size_t grid_stride) {
  const size_t one = gf_layout(1, w, h, grid_stride).total + 1024;  // (the sections' alignment: < 1024 bytes)
  const size_t fit = std::max<size_t>((c->gf_ws.bytes - 1024) / one, 1);
  const int m = (int)std::min<size_t>(fit, (size_t)n);
  const int slices = (n + m - 1) / m;
  return (n + slices - 1) / slices;  // even slices
}

// enqueues the three stages for n device frames; the results go to gf_res (counts | corners)
int gf_run(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
           const GfArgs& a, hipStream_t s) {
  int st = gf_enter(c, s);
  if (st != ORBX_OK) return st;
  const GfMark mark{c, s};
  c->gf_n = 0;  // (a failed call leaves no "last batch")
  if ((st = gf_workspace(c)) != ORBX_OK) return st;
  const size_t o_corners = align_up_sz(sizeof(int32_t) * (size_t)n, 256);
  const size_t res_bytes = o_corners + sizeof(float) * 2 * (size_t)a.cap * n;
  if (c->gf_res.p && c->gf_res.bytes < res_bytes && (st = gf_wait(c)) != ORBX_OK) return st;  // (still written?)
  ENSURE(c, c->gf_res, res_bytes);
  const size_t grid_stride = a.suppress ? (size_t)a.gw * a.gh * a.slots : 0;
  const int per = gf_slice_frames(c, n, w, h, grid_stride);
  int32_t* d_counts = (int32_t*)c->gf_res.p;
  float* d_corners = (float*)((uint8_t*)c->gf_res.p + o_corners);
  for (int f0 = 0; f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    const GfLayout L = gf_layout(m, w, h, grid_stride);
    uint8_t* ws = (uint8_t*)c->gf_ws.p;
    uint32_t* d_max = (uint32_t*)(ws + L.cnt);
    int32_t* d_ncand = (int32_t*)(d_max + m);
    HIPCHK(c, hipMemsetAsync(d_max, 0, 2 * sizeof(uint32_t) * (size_t)m, s));
    if (a.suppress) HIPCHK(c, hipMemsetAsync(ws + L.grid, 0xff, sizeof(uint32_t) * grid_stride * m, s));
    HIPCHK(c, orbx_launch_gftt_response(s, d_frames + frame_stride * (size_t)f0, m, w, h, row_stride, frame_stride,
                                        (float*)(ws + L.map), d_max));
    HIPCHK(c, orbx_launch_gftt_candidates(s, (const float*)(ws + L.map), m, w, h, d_max, a.quality,
                                          (unsigned long long*)(ws + L.keys), L.pool, d_ncand));
    HIPCHK(c, orbx_launch_gftt_select(s, m, w, (unsigned long long*)(ws + L.keys), L.pool, d_ncand, a.min_distance,
                                      a.cell, a.gw, a.gh, a.slots, (uint32_t*)(ws + L.grid), grid_stride, a.cap,
                                      d_counts + f0, d_corners + (size_t)2 * a.cap * f0));
  }
  c->gf_n = n;
  c->gf_cap = a.cap;
  return ORBX_OK;
}

// a host image, tightly packed, in gf_img on the context's stream
int gf_upload(orbx_ctx* c, const uint8_t* image, int w, int h, int stride) {
  int st = gf_enter(c, c->stream);
  if (st != ORBX_OK) return st;
  const GfMark mark{c, c->stream};
  ENSURE(c, c->gf_img, (size_t)w * h);
  HIPCHK(c, hipMemcpy2DAsync(c->gf_img.p, w, image, stride, w, h, hipMemcpyHostToDevice, c->stream));
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_corner_min_eigen_val(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, float* eig) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!eig) return fail(c, ORBX_ERR_INVALID_ARG, "eig is NULL");
  if ((st = gf_upload(c, image, width, height, stride)) != ORBX_OK) return st;
  const GfMark mark{c, c->stream};
  if ((st = gf_workspace(c)) != ORBX_OK) return st;
  const GfLayout L = gf_layout(1, width, height, 0);
  uint8_t* ws = (uint8_t*)c->gf_ws.p;
  HIPCHK(c, hipMemsetAsync(ws + L.cnt, 0, 2 * sizeof(uint32_t), c->stream));
  HIPCHK(c, orbx_launch_gftt_response(c->stream, (const uint8_t*)c->gf_img.p, 1, width, height, width,
                                      (size_t)width * height, (float*)(ws + L.map), (uint32_t*)(ws + L.cnt)));
  HIPCHK(c, hipMemcpyAsync(eig, ws + L.map, sizeof(float) * (size_t)width * height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_good_features_to_track(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int max_corners,
                                double quality_level, double min_distance, float* corners_xy, int capacity,
                                int* count) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!count || capacity < 0 || (capacity > 0 && !corners_xy))
    return fail(c, ORBX_ERR_INVALID_ARG, "count / corners_xy is NULL or capacity < 0");
  if ((st = gf_check_params(c, quality_level, min_distance)) != ORBX_OK) return st;
  if ((st = gf_upload(c, image, width, height, stride)) != ORBX_OK) return st;
  const GfArgs a = gf_args(width, height, max_corners, quality_level, min_distance);
  if ((st = gf_run(c, (const uint8_t*)c->gf_img.p, 1, width, height, width, (size_t)width * height, a, c->stream)) !=
      ORBX_OK)
    return st;
  int32_t found = 0;
  HIPCHK(c, hipMemcpyAsync(&found, c->gf_res.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (found > capacity) {
    *count = found;
    return fail(c, ORBX_ERR_CAPACITY, "corners_xy is too small");
  }
  if (found > 0)
    HIPCHK(c, hipMemcpy(corners_xy, (const uint8_t*)c->gf_res.p + align_up_sz(sizeof(int32_t), 256),
                        sizeof(float) * 2 * (size_t)found, hipMemcpyDeviceToHost));
  *count = found;
  return ORBX_OK;
}

int orbx_good_features_batch_device(orbx_ctx* c, const void* d_frames, int n, int width, int height, int row_stride,
                                    size_t frame_stride, int max_corners, double quality_level, double min_distance,
                                    void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!d_frames) return fail(c, ORBX_ERR_INVALID_ARG, "d_frames is NULL");
  if (n < 1 || n > c->p.max_batch) return fail(c, ORBX_ERR_INVALID_ARG, "n outside [1, max_batch]");
  if (width < 8 || height < 8 || width > c->p.max_width || height > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "image size outside [8, max_width] x [8, max_height]");
  if (row_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "row_stride < width");
  if (frame_stride < (size_t)row_stride * (size_t)(height - 1) + (size_t)width)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame_stride smaller than a frame");
  // the kernel addresses the bytes of one frame with 32-bit offsets (a buffer descriptor per frame)
  if ((unsigned long long)row_stride * (unsigned long long)(height - 1) + (unsigned long long)width > 0x7fffffffull)
    return fail(c, ORBX_ERR_INVALID_ARG, "row_stride * (height - 1) + width exceeds 2^31 - 1");
  if (max_corners < 1) return fail(c, ORBX_ERR_INVALID_ARG, "max_corners < 1");
  const int st = gf_check_params(c, quality_level, min_distance);
  if (st != ORBX_OK) return st;
  return gf_run(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride,
                gf_args(width, height, max_corners, quality_level, min_distance),
                stream ? (hipStream_t)stream : c->stream);
}

int orbx_good_features_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = gf_wait(c);
  if (st != ORBX_OK) return st;
  if (c->gf_ws.p) {
    HIPCHK(c, hipFree(c->gf_ws.p));
    c->gf_ws = DevBuf{};
  }
  c->gf_ws_limit = bytes ? bytes : ORBX_GFTT_WORKSPACE_DEFAULT;
  return ORBX_OK;
}

int orbx_good_features_results_device(orbx_ctx* c, orbx_good_features_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->gf_n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  v->counts = (const int32_t*)c->gf_res.p;
  v->corners_xy = (const float*)((const uint8_t*)c->gf_res.p + align_up_sz(sizeof(int32_t) * (size_t)c->gf_n, 256));
  v->slot_capacity = c->gf_cap;
  v->n = c->gf_n;
  return ORBX_OK;
}

int orbx_good_features_fetch(orbx_ctx* c, int first, int n, int32_t* counts, float* corners_xy) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->gf_n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  if (!counts || first < 0 || n < 1 || first >= c->gf_n || n > c->gf_n - first)
    return fail(c, ORBX_ERR_INVALID_ARG, "counts is NULL or [first, first + n) outside the batch");
  const int st = gf_wait(c);
  if (st != ORBX_OK) return st;
  const uint8_t* res = (const uint8_t*)c->gf_res.p;
  HIPCHK(c, hipMemcpy(counts, res + sizeof(int32_t) * (size_t)first, sizeof(int32_t) * (size_t)n,
                      hipMemcpyDeviceToHost));
  if (corners_xy) {
    const size_t row = sizeof(float) * 2 * (size_t)c->gf_cap;
    HIPCHK(c, hipMemcpy(corners_xy, res + align_up_sz(sizeof(int32_t) * (size_t)c->gf_n, 256) + row * first, row * n,
                        hipMemcpyDeviceToHost));
  }
  return ORBX_OK;
}

}  // extern "C"
