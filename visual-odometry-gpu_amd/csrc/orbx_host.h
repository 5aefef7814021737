// orbx_host.h -- what every part of the C-ABI host layer (orbx_api*.cpp) shares: the context and the records it is
// made of, the error and device guards, and the helpers that more than one of those files calls (defined once, in
// orbx_api.cpp).  Every part owns a few blocks whose sections orbx_layout.h places.  The blocks of the work beside the
// batched path grow through SideWork::grow; ensure() grows those of the paths that run on the context's stream or the
// last batch's: the stage scratch, the matcher, the pair tracker, pose, scale and bundle adjustment of staged windows.
// Host only: included by no .hip file, and not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/orbx_reloc.h"
#include "orbx_internal.h"
#include "orbx_layout.h"
#include "orbx_tables.h"

namespace orbx_host {

using namespace orbx_geom;    // orbx_plan.h: the geometry of a frame size and the tables built from it
using namespace orbx_layout;  // orbx_layout.h: the sections of every block

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
// section `off` of a block, as the array of T that a launch or a copy takes
template <class T>
T* at(const DevBuf& b, size_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(b.p) + off); }
// what a subsystem's release() does with the buffers it owns (nothing may still be using them)
inline void free_bufs(std::initializer_list<DevBuf*> bufs) {
  for (DevBuf* b : bufs)
    if (b->p) (void)hipFree(b->p);
}

// One block of the ring of result blocks (orbx_ctx::blocks): the device allocation (OutLayout of orbx_layout.h), its
// pinned host mirror -- a whole batch comes back with a single D2H copy -- and what the batch that last wrote it left
// there.
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

// a per-workgroup tile descriptor table (see OrbxTileDesc; T_* of orbx_tables.h) of the current plan, in a pool sized
// for the largest frame (orbx_ctx::table_cap)
struct TileTable {
  OrbxTileDesc* d = nullptr;
  int count = 0;
};

// the events of one timed batched call
// (slots ORBX_NUM_STAGE_TIMES + 1, + 2: the boundaries inside the top-rows-first pipeline)
struct TimingSet {
  hipEvent_t ev[ORBX_NUM_STAGE_TIMES + 3] = {};
  int mode = 0;
  bool split = false;  // the call ran the top-rows-first pipeline
};

int fail(orbx_ctx* c, int status, const std::string& msg);  // (c == NULL: the thread's creation error)

#define HIPCHK(c, expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return fail((c), ORBX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

// Work that runs beside the batched path on ANY caller's stream, with one workspace and one result block per context
// (good features, LK windows, landmarks, tracks pose, window poses).  `stream` is the stream the last call ran on,
// kept for COMPARISON only (a caller's stream may be gone by the next call); `ev` is recorded behind that call's
// work: what later calls, fetches and orbx_destroy wait for.
struct SideWork {
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;
  // waits for the work enqueued so far, on whatever stream it ran: through the event recorded behind it, never
  // through the stream itself (a caller's stream need not outlive its batch's end)
  int wait(orbx_ctx* c);
  // a call on stream s: earlier work on another stream has to be done (one workspace, one result block)
  int enter(orbx_ctx* c, hipStream_t s);
  // a call on s reads what `producer` left, perhaps on another stream: s waits for the producer's event
  int after(orbx_ctx* c, const SideWork& producer, hipStream_t s);
  // a buffer of this work of at least `bytes`.  One that grows first waits for the event (the old allocation may
  // still be read or written); the new allocation is made BEFORE the old one is released, so that a failed call
  // keeps what it had
  int grow(orbx_ctx* c, DevBuf& b, size_t bytes);
  // records the event behind whatever a call has enqueued on s, on every way out of the call
  struct Mark {
    SideWork& w;
    hipStream_t s;
    ~Mark() {
      if (w.ev) (void)hipEventRecord(w.ev, s);
    }
  };
  // the last wait, and the end of the event (orbx_destroy, before the owner's buffers are freed)
  void release() {
    if (!ev) return;
    (void)hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
  }
};

// A small host table that goes up through a pinned mirror (a copy from pageable memory would make the host wait for
// the stream).  The mirror is reused: `ev` is recorded behind every copy, and the next one first waits for it.
struct PinnedUpload {
  void* host = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  int send(orbx_ctx* c, void* d_dst, const void* src, size_t n, hipStream_t s);
  void release() {
    if (ev) (void)hipEventDestroy(ev);
    if (host) (void)hipHostFree(host);
  }
};

// ---- the context's parts, one per subsystem (orbx_ctx::s, m, lk, lkw, pose, scale, ba, gf, lm, tp, wp, st) ----

// stage-API scratch (grown on demand; never touched by the batched path)
struct StageScratch {
  DevBuf img_a, img_b, f32, u16, mask, kps, f32b, desc, i32, kern;
  DevBuf tiles;  // stage-API tables
  void release() { free_bufs({&img_a, &img_b, &f32, &u16, &mask, &kps, &f32b, &desc, &i32, &kern, &tiles}); }
};

// descriptor matcher: ONE result block (MatchBlock of orbx_layout.h) that the host-array entry and the batch entry
// share, and the staged input of the host-array entry (MatchInput)
struct Matcher {
  DevBuf res, in;
  int pairs = 0, cap = 0;  // pairs and slots per pair of the batch match the block holds (pairs == 0: none)
  long long serial = -1;  // the batch serial (orbx_ctx::batch_serial) the last batch match was made on
  // bumped by every batch match: the pose step records the one it read (Pose::match_gen), so the scale step, which
  // reads m.match again, can tell that the matches are still the ones the poses were computed from
  long long gen = 0;
  void release() { free_bufs({&res, &in}); }
};

// Lucas-Kanade tracker: two image pyramids (ping-pong: the `next` of one call is the
// `prev` of the following one), the derivative pyramid of the current `prev`, point buffers
struct LkPair {
  DevBuf img[2], deriv, io;  // io: the point block (LkIo of orbx_layout.h)
  void* host = nullptr;      // pinned mirror of io (one H2D + one D2H per call)
  size_t host_bytes = 0;
  int w = 0, h = 0, top = -1, win = 0, last = -1;  // last: buffer holding the last `next`
  void release() {
    if (host) (void)hipHostFree(host);
    free_bufs({&img[0], &img[1], &deriv, &io});
  }
};

// Lucas-Kanade over frame windows (k_lk_track_windows): the workspace of one slice of frames, bounded by ws_limit;
// the window table; the staged frames and points of the one-window host entry; and the entry's OWN result block
// (LkwLayout, LkwResult of orbx_layout.h).  A call with the forward-backward check (rank 13) writes the same block
// and, beside it, fb_d2 | lost into a buffer of their own (fbres, LkwFbResult).  Nothing here is shared with
// orbx_lk_track.
struct LkWindows {
  DevBuf ws, first, img, pts, res, fbres;
  size_t ws_limit = ORBX_LK_WORKSPACE_DEFAULT;
  int n = 0, cap = 0, len = 0;  // windows, slots per window, frames per window of the last call (0: none)
  bool fb = false;              // the last call ran the forward-backward check: fbres belongs to it
  SideWork side;                // the event is recorded behind every windows call
  PinnedUpload first_up;        // the window table's way up
  void release() {
    side.release();
    first_up.release();
    free_bufs({&ws, &first, &img, &pts, &res, &fbres});
  }
};

// relative pose (orbx_pose.hip): the batch entry's block (PoseBlock of pairs x cap), and the host-array entry's own
// block (PoseBlock of one pair) with its staged point lists
struct Pose {
  DevBuf blk, hblk, hin;
  int pairs = 0, cap = 0;
  hipStream_t stream = nullptr;
  long long serial = -1;     // the batch serial the last batch pose ran on
  long long match_gen = -1;  // the Matcher::gen it read
  void release() { free_bufs({&blk, &hblk, &hin}); }
};

// triangulation and scale (orbx_scale.hip): the batch entry's block (ScaleBlock of pairs x cap), and the one buffer
// the two host-array entries lay out in turn (TriHost, ScaleHost)
struct Scale {
  DevBuf blk, host;
  int pairs = 0, cap = 0;
  hipStream_t stream = nullptr;
  void release() { free_bufs({&blk, &host}); }
};

// bundle adjustment of staged windows (orbx_ba.hip): the windows and their summaries (BaStage of orbx_layout.h) and
// the workgroups' workspaces (LmWork); grown on first use
struct BundleAdjust {
  DevBuf stage, ws, prior;  // prior: [points][4] of a call with landmark priors (rank 20)
  void release() { free_bufs({&stage, &ws, &prior}); }
};

// landmarks of tracked windows and their bundle adjustment on the device (orbx_landmarks.hip, orbx_ba.hip): the
// scratch of a build, the entry's OWN result block (what k_ba_lm reads), the solve's copies of poses and points with
// its summaries, the solve's workspaces (LmScratch, LmBlock, LmSolve, LmWork of orbx_layout.h), and the staged tracks
// of the one-window host entry.  A build from every view of a track (rank 15) writes the same block and, beside it,
// its table of view records and reason | reproj_px into a buffer of their own (views, LmViews).  Nothing here is
// shared with orbx_bundle_adjust_batch.
struct Landmarks {
  DevBuf scr, blk, sol, ws, stage, views;
  double K[9] = {};
  int n = 0, cap = 0, len = 0;  // windows, slots per window, poses per window of the last build (0: none)
  bool has_views = false;       // the last build was a views build: `views` belongs to it
  bool solved = false;          // the block has been solved since it was built
  long long gen = 0;            // bumped by every build: what the PnP batch records (Pnp::lm_gen)
  SideWork side;                // the event is recorded behind every build and every solve
  PinnedUpload poses_up;        // the pose table's way up
  void release() {
    side.release();
    poses_up.release();
    free_bufs({&scr, &blk, &sol, &ws, &stage, &views});
  }
};

// pose and scale of tracked frame pairs (orbx_tracks.hip, k_pose_ransac, k_scale_join): the normalised point lists
// (scratch), the entry's OWN result block (TpBlock of orbx_layout.h), and the staged tracks of the one-window host
// entry.  Nothing here is shared with the batch pose / scale entries.
struct TracksPose {
  DevBuf scr, blk, stage;
  int n = 0, cap = 0, len = 0;  // windows, slots per window, frames per window of the last call (0: none)
  SideWork side;                // the event is recorded behind every call
  void release() {
    side.release();
    free_bufs({&scr, &blk, &stage});
  }
};

// window poses chained from the tracks-pose block and the write-back gate behind a solve (orbx_wposes.hip): what goes
// up with a chain (WpInput of orbx_layout.h), the chain's OWN result block (WpBlock), the gate's OWN result block
// (WbBlock), and the staged tracks of the one-window host entry.  The chain reads tp.blk, the gate reads lm.scr and
// lm.sol, and the chained landmarks build reads blk; none of them writes there.
struct WindowPoses {
  DevBuf in, blk, wb, stage;
  int n = 0, len = 0;        // windows and frames per window of the last chain (0: none)
  int wb_n = 0, wb_len = 0;  // the same of the last write-back
  SideWork side;             // the event is recorded behind every chain and every write-back
  PinnedUpload up;           // T0 | scale0 on their way up
  void release() {
    side.release();
    up.release();
    free_bufs({&in, &blk, &wb, &stage});
  }
};

// overlapping windows joined into one trajectory (orbx_stitch.hip): what goes up with a stitch and what its kernels
// hand one another (StInput of orbx_layout.h), the stitch's OWN result block (StBlock), and the staged tracks of the
// host stream entry.  The stitch reads the caller's poses -- wp.blk or wp.wb when they are a view of those -- and
// writes nowhere else.
struct StreamStitch {
  DevBuf in, blk, stage;
  int n = 0, len = 0, stride = 0;  // windows, frames per window and stride of the last stitch (n == 0: none)
  SideWork side;                   // the event is recorded behind every stitch
  PinnedUpload up;                 // T_start on its way up
  void release() {
    side.release();
    up.release();
    free_bufs({&in, &blk, &stage});
  }
};

// perspective-n-point over the landmarks block (orbx_pnp.hip): the gathered correspondences (PnpScratch of
// orbx_layout.h) and the entry's OWN result block (PnpBlock), and the same pair for the one problem of the host-array
// entry.  The batch reads lm.blk and lm.scr; the seeded solve reads blk's poses.  Nothing is written elsewhere.
struct Pnp {
  DevBuf scr, blk, hscr, hblk;
  int n = 0, cap = 0, len = 0;  // windows, slots per window, frames per window of the last batch (0: none)
  long long lm_gen = -1;        // the Landmarks::gen of the block the last batch read
  SideWork side;                // the event is recorded behind every call
  void release() {
    side.release();
    free_bufs({&scr, &blk, &hscr, &hblk});
  }
};

// landmarks carried into the next generation of windows and the PnP of every frame of those windows against them
// (orbx_carry.hip, k_pnp_ransac; rank 18): the carry block (CarryBlock of orbx_layout.h), the carried PnP's scratch and
// its OWN result block (CarryPnpScratch, CarryPnpBlock), and the staged arrays of the one-window host entry
// (CarryStage).  The carry reads lm.blk or lm.sol and the caller's origin; the carried PnP reads blk and the caller's
// tracks; the carried landmarks build reads pblk.  Nothing is written elsewhere.
struct Carry {
  DevBuf blk, pscr, pblk, stage;
  int n = 0, cap = 0;              // windows and slots per window of the last carry (0: none)
  int pn = 0, pcap = 0, plen = 0;  // windows, slots and frames per window of the last carried PnP (0: none)
  SideWork side;                   // the event is recorded behind every carry and every carried PnP
  void release() {
    side.release();
    free_bufs({&blk, &pscr, &pblk, &stage});
  }
};

// landmark priors of a carried window (orbx_prior.hip; rank 20): the priors' OWN block (PriorBlock of orbx_layout.h),
// gathered from lm.blk and carry.blk; the solve with priors reads it.  It runs under the landmarks' event (lm.side),
// as the builds and solves of the block it belongs to do.
struct Priors {
  DevBuf blk;
  int n = 0, cap = 0;     // windows and slots per window of the landmarks block it was gathered for (0: none)
  long long lm_gen = -1;  // the Landmarks::gen of that block
  void release() { free_bufs({&blk}); }
};

// descriptors at caller-held points and the re-association of two described sets (orbx_reloc.hip; rank 19): the
// level-0 frames of one slice (ws, bounded by ws_limit), the OK slots of every frame in slot order (list), the two
// banks' OWN result blocks (PdBlock of orbx_layout.h), the staged image and points of the one-image host entry
// (PdStage); the re-association's scratch (the best key per train slot), its OWN result block (RaBlock) and the staged
// sets of the one-window host entry (RaStage).  The describe reads the caller's frames and points, the re-association
// the caller's descriptors and states -- the banks, when they are views of those; nothing is written elsewhere.
struct Reloc {
  DevBuf ws, list, bank[2], stage, best, rblk, rstage;
  size_t ws_limit = ORBX_PD_WORKSPACE_DEFAULT;
  int n[2] = {0, 0}, cap[2] = {0, 0};  // frames and slots per frame of each bank (n == 0: not written)
  int rn = 0, rq = 0, rt = 0;          // windows, query and train slots of the last re-association (rn == 0: none)
  SideWork side;                       // the event is recorded behind every describe and every re-association
  void release() {
    side.release();
    free_bufs({&ws, &list, &bank[0], &bank[1], &stage, &best, &rblk, &rstage});
  }
};

// the search by projection (orbx_search.hip; rank 21): the projection's OWN result block (SpBlock of orbx_layout.h)
// and the staged arrays of its one-window host entry (SpStage), under an event of their own; the gated
// re-association's scratch (SgScratch), its candidates block (SgBlock) and the staged sets of its one-window host entry
// (SgStage), which run under the re-association's event (Reloc::side): the gated call replaces Reloc::rblk.  The
// projection reads lm.blk or lm.sol and the caller's poses; the gated call reads the caller's arrays -- the banks and
// the projection block, when they are views of those; nothing is written elsewhere.
struct Search {
  DevBuf blk, stage, gscr, gblk, gstage;
  int n = 0, cap = 0;    // windows and old slots per window of the last projection (0: none)
  int gn = 0, gq = 0;    // windows and query slots of the last gated re-association (0: none)
  SideWork side;         // the event is recorded behind every projection
  void release() {
    side.release();
    free_bufs({&blk, &stage, &gscr, &gblk, &gstage});
  }
};

// Shi-Tomasi corners (orbx_gftt.hip): the workspace of one slice of frames, allocated on first use and bounded by
// ws_limit; the staged host image of the one-frame entries; and the entry's OWN result block, untouched by the ORB
// path.  Rank 12 (top-up and masked detection) adds, beside the workspace and for the same number of frames, the bit
// maps of blocked pixels (bm: allocated at the first top-up or masked call, freed with the workspace), the staged
// seeds or mask of the host entries, and a result block of its own (tres).  Gf-, Gr-, Gb-, GtLayout of orbx_layout.h.
struct GoodFeatures {
  DevBuf ws, img, res, bm, stage, tres;
  size_t ws_limit = ORBX_GFTT_WORKSPACE_DEFAULT;
  int n = 0, cap = 0;    // frames and slots per frame of the last good-features batch (n == 0: none)
  int tn = 0, tcap = 0;  // the same of the last top-up
  SideWork side;
  void release() {
    side.release();
    free_bufs({&ws, &img, &res, &bm, &stage, &tres});
  }
};

}  // namespace orbx_host

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
  orbx_host::TileTable tiles[kTileTables];
  OrbxTopLevels top_levels{};  // the levels the second pass may skip
  std::vector<OrbxResizeTap> h_taps;
  OrbxPlanTables scratch;        // set_plan builds the next size's tables here (a re-tile reuses the vectors)
  orbx_geom::OrbxTableCapacity table_cap{};  // entries of the table pools and of d_taps (orbx_plan.h: table_capacity)
  int plan_w = 0, plan_h = 0;

  uint8_t* d_in = nullptr;  // staged host frames, tight pitch (max_batch frames of max_width x max_height)
  // captured launch sequences of the most recent batch shapes (run_batch), round-robin replacement
  static constexpr int kGraphs = 16;  // (input, result block, lane) triples: 8 resident inputs over 4 blocks x 2 lanes
  hipGraphExec_t g_exec[kGraphs] = {};
  OrbxGraphKey g_key[kGraphs] = {};
  int g_next = 0;
  int plan_serial = 0;  // bumped whenever set_plan rebuilds the plan / tables
  OrbxResizeTap* d_taps = nullptr;
  float* d_gauss = nullptr;
  // Result blocks.  A ring of kBlocks, used in turn by consecutive batches, each with a pinned host
  // mirror: the D2H copy of batch i (orbx_batch_prefetch, on its own copy stream) overlaps the
  // kernels of batch i+1, which write the other block.  blocks[blk] is the block of the most recent batch.
  // (a ring of kBlocks blocks: with two, the copy of batch i -- about as long as a step at 256 frames per batch --
  // had to finish before batch i + 2 could start; with four it overlaps two following batches)
  static constexpr int kBlocks = 4;
  orbx_host::Block blocks[kBlocks];
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
  orbx_host::Lane lanes[2];
  int lane = 0;
  bool pipelined = false;
  bool last_two_pass = false;  // the last batch built its pyramid top rows first (enqueue_batch)
  hipStream_t last_stream = nullptr;

  long long batch_serial = 0;  // bumped by every batch run
  // The subsystems beside the batched path, each with what it owns.  They meet in five places, visible where the
  // calls are made: pose reads the matcher's table, scale checks pose.match_gen against m.gen, the windows
  // tracker waits for the good-features event, the landmarks build and the tracks pose wait for the windows
  // tracker's, the window poses wait for the tracks pose's, the chained landmarks build for the window poses', and
  // the write-back gate for the solve's, and the stitch for the window poses' (chain and gate share one event); the
  // PnP batch waits for the landmarks' event (build and solve share one) and the seeded solve for the PnP batch's; the
  // carry waits for the landmarks' and the top-up's, the carried PnP for the windows tracker's, and the carried
  // landmarks build for the carried PnP's (carry and carried PnP share one event); the point descriptors wait for the
  // good features' and the windows tracker's, and the carry also for the re-association's (describe and
  // re-association share one event); the projection waits for the landmarks', the carry's and the window poses'
  // events (its poses may be theirs), and the gated re-association for the projection's, the good features' and the
  // windows tracker's.
  orbx_host::StageScratch s;
  orbx_host::Matcher m;
  orbx_host::LkPair lk;
  orbx_host::LkWindows lkw;
  orbx_host::Pose pose;
  orbx_host::Scale scale;
  orbx_host::BundleAdjust ba;
  orbx_host::GoodFeatures gf;
  orbx_host::Landmarks lm;
  orbx_host::TracksPose tp;
  orbx_host::WindowPoses wp;
  orbx_host::StreamStitch st;
  orbx_host::Pnp pnp;
  orbx_host::Carry carry;
  orbx_host::Reloc reloc;
  orbx_host::Priors prior;
  orbx_host::Search search;

  int timing = 0;  // 0 off, 1 all stages, 2 blur + fast only
  int fast_early = 1;
  int blur_impl = 2;  // ORBX_BLUR_IMPL, read at creation (launch_blur_auto)
  int fast_impl = 4;  // 4: streaming kernel (orbx_fast4.hip, the default), 3: LDS tile kernel (orbx_fast.hip); ORBX_FAST_IMPL, read at creation
  int fuse = 1;  // pyramid + blur in one kernel when blur runs on every level (orbx_set_fused_pyramid_blur)
  // the scheduler of the first pass (orbx_adapt.h): what it has learned and its switches, and the words the device
  // reports into -- running totals and per-level fill rows (ORBX_FEEDBACK_WORDS, orbx_plan.h), written to the pinned
  // h_feedback by the last kernel of every two-pass batch and read WITHOUT waiting at the start of later ones
  OrbxAdapt adapt;
  uint32_t* d_feedback = nullptr;
  volatile uint32_t* h_feedback = nullptr;
  // ring of event sets: one per timed batched call, so that several calls can be
  // in flight before their stage times are read (no host sync between steps)
  orbx_host::TimingSet evr[ORBX_EVENT_SETS];
  long long ev_calls = 0;  // timed batched calls so far
  hipEvent_t ev[2] = {};   // orbx_bench_stage
};

namespace orbx_host {

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

// a buffer of at least `bytes`; one that grows first waits for the context's stream, both lanes and the last
// batch's stream (the buffers of the work beside the batched path have waits of their own: SideWork)
int ensure(orbx_ctx* c, DevBuf& b, size_t bytes);
#define ENSURE(c, buf, bytes)                        \
  do {                                               \
    const int _st = ensure((c), (buf), (bytes));     \
    if (_st != ORBX_OK) return _st;                  \
  } while (0)

// the stream the last batch ran on (the context's own before any batch)
hipStream_t batch_stream(const orbx_ctx* c);
// the lane and the result block of the most recent batch
const Lane& cur_lane(const orbx_ctx* c);
const Block& last_block(const orbx_ctx* c);
// everything either lane has in flight has finished
hipError_t lanes_sync(orbx_ctx* c);

int check_image(orbx_ctx* c, const void* img, int w, int h, int stride);
// An array of n frames on the device, n in [n_min, n_max]: pointer, count, size against the context's maximum,
// strides, and the 2^31 - 1 bound of the kernels' 32-bit frame offsets (a buffer descriptor per frame).  `what`
// carries the caller's words for its pointer and its count.
struct FramesWhat {
  const char* null_msg;
  std::string range_msg;
};
int check_device_frames(orbx_ctx* c, const void* d_frames, int n, int n_min, int n_max, int w, int h, int row_stride,
                        size_t frame_stride, const FramesWhat& what);
bool finite_all(const double* v, int n);
// the argument rules of every relative-pose entry (include/orbx.h, rank 5), and one pair's result taken apart
inline bool pose_args_ok(const double* K, double prob, double threshold, int max_iters) {
  return K && K[0] > 0 && K[4] > 0 && std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) &&
         std::isfinite(K[5]) && std::isfinite(prob) && std::isfinite(threshold) && threshold >= 0 && max_iters >= 0 &&
         max_iters <= ORBX_POSE_MAX_ITERS;
}
inline void pose_unpack(const OrbxPoseOut& r, double* E, double* R, double* t, int32_t* inliers, int32_t* good,
                        int32_t* iters) {
  if (E) memcpy(E, r.E, sizeof r.E);
  if (R) memcpy(R, r.R, sizeof r.R);
  if (t) memcpy(t, r.t, sizeof r.t);
  if (inliers) *inliers = r.inliers;
  if (good) *good = r.good;
  if (iters) *iters = r.iters;
}
int gaussian_kernel(int K, float sigma, float* kernel);
hipError_t launch_blur_auto(int impl, hipStream_t s, const OrbxPlan& P, const OrbxTileMap& tm1, const OrbxTileDesc* tiles2,
                            int ntiles2, int n, const uint8_t* src, uint8_t* dst, int first_level, int kind);
// behind both *_workspace_limit entries: the users of the workspace (and of what is sized with it) have finished, it
// is released (the next call allocates one within the new limit), and the limit becomes `bytes`, or `dflt` for 0
int set_workspace_limit(orbx_ctx* c, SideWork& side, std::initializer_list<DevBuf*> ws, size_t* limit, size_t bytes,
                        size_t dflt);
// the stream an entry runs on: the caller's, or the context's own for NULL
inline hipStream_t stream_of(const orbx_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }
// [first, first + n) lies inside [0, total) and has at least n_min elements
inline bool range_ok(int first, int n, int total, int n_min = 1) {
  return first >= 0 && n >= n_min && n <= total - first;
}
// one window's tracks | seen from host arrays into `stage`, on the context's stream (the one-window host entries)
int stage_tracks(orbx_ctx* c, SideWork& side, DevBuf& stage, const float* tracks_xy, const int32_t* seen, int n_slots,
                 int window_len, const float** d_tracks, const int32_t** d_seen);
// the landmarks build behind its two entries (orbx_api_landmarks.cpp).  lm_check_build: the argument rules; the poses
// are checked when they come from the host (poses6 != NULL).  lm_run enqueues the build on s with the poses from the
// host (poses6, through the pinned mirror) or from the window-poses block (poses6 == NULL: d_poses6 and d_pose_status,
// copied on s behind that block's event).  views: NULL for the build of rank 10, else the options of the build from
// every view of a track (rank 15), checked by lm_views_ok.  producer: the work that wrote d_poses6 when that is not the
// window-poses block (the carried PnP, rank 18)
struct LmViewsOptions {
  int tri_mode;
  double max_reproj_px;
};
bool lm_views_ok(const LmViewsOptions& o);
bool ba_params_ok(double huber_delta, int max_iters);
int lm_check_build(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len,
                   const double* poses6);
int lm_run(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
           const double* poses6, const double* d_poses6, const int32_t* d_pose_status, hipStream_t s,
           const LmViewsOptions* views = nullptr, const SideWork* producer = nullptr);
// the argument rules of orbx_tracks_pose_device (orbx_api_tracks.cpp)
int tp_check(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len, double prob,
             double threshold, int max_iters);
// the chain of the last tracks-pose block on s behind its two entries (orbx_api_wposes.cpp).  T0 / scale0: host or
// NULL.  stream_of_windows: NULL, or the chain of a stream of overlapping windows (rank 16): T0 and scale0 have to be
// NULL, every window starts at the identity, and scale0 is gathered on the device from the tracks-pose block itself
struct WpStreamOptions {
  int stride;
  double scale0_first;
};
int wp_check(orbx_ctx* c, const double* T0, const double* scale0, const WpStreamOptions* stream_of_windows);
int wp_run(orbx_ctx* c, const double* T0, const double* scale0, hipStream_t s,
           const WpStreamOptions* stream_of_windows = nullptr);
bool gate_params_ok(double max_rot, double max_trans);
// the solve of the landmarks block on s behind orbx_bundle_adjust_landmarks_device and its PnP-seeded twin
// (orbx_api_landmarks.cpp): d_poses6 is what the solve's poses copy is taken from -- NULL: the poses the block was
// built from -- and `producer`, when not NULL, the work that wrote them, perhaps on another stream
// d_prior, when not NULL: [points][4] in the block's point order, and the solve is the one with landmark priors
// (rank 20) from `start`, an orbx_prior_start
int lm_solve(orbx_ctx* c, double huber_delta, int max_iters, hipStream_t s, const double* d_poses6,
             const SideWork* producer, const double* d_prior = nullptr, int start = 0);
// the staged solve behind orbx_bundle_adjust_batch (orbx_api_geom.cpp) and, with `prior`, behind
// orbx_bundle_adjust_prior_batch (orbx_api_prior.cpp): xyz / weight both NULL means every weight is 0
struct BaPriorArgs {
  const double *xyz, *weight;
  int start;
};
int ba_batch(orbx_ctx* c, const double* K, int n_windows, const int32_t* pose_offset, double* poses6,
             const int32_t* point_offset, double* points3, const int32_t* obs_offset, const int32_t* obs_point,
             const int32_t* obs_pose, const double* obs_xy, double huber_delta, int max_iters,
             orbx_ba_summary* summaries, const BaPriorArgs* prior);

}  // namespace orbx_host
