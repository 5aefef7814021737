// orbx_api.cpp -- C-ABI host layer of liborbx.so (see include/orbx.h): the context and the batched ORB path.
//
// Owns the context (device memory pools, stream, per-size plan), validates
// arguments, sequences the kernel launches of orbx_kernels.hip and moves
// results.  The subsystems beside the batched path are driven from files of their own, on the context and the
// helpers of orbx_host.h: orbx_api_stage.cpp (stage operators, matcher), orbx_api_lk.cpp (Lucas-Kanade),
// orbx_api_geom.cpp (pose, scale, bundle adjustment), orbx_api_gftt.cpp (good features).  There is NO CPU fallback
// anywhere in the host layer: if the HIP runtime or a gfx950 device is missing every entry point fails loudly with
// ORBX_ERR_NO_DEVICE / ORBX_ERR_HIP.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "orbx_host.h"

using namespace orbx_host;
using namespace orbx_tables;  // (and through it orbx_adapt)

namespace {
thread_local std::string g_create_error;
}  // namespace

// ---- what the other files of the host layer call too (declared in orbx_host.h) ----
namespace orbx_host {

int fail(orbx_ctx* c, int status, const std::string& msg) {
  if (c)
    c->err = msg;
  else
    g_create_error = msg;
  return status;
}

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

hipStream_t batch_stream(const orbx_ctx* c) { return c->last_stream ? c->last_stream : c->stream; }
const Lane& cur_lane(const orbx_ctx* c) { return c->lanes[c->lane]; }
const Block& last_block(const orbx_ctx* c) { return c->blocks[c->blk]; }
hipError_t lanes_sync(orbx_ctx* c) {
  for (const Lane& L : c->lanes)
    if (L.stream) {
      const hipError_t e = hipStreamSynchronize(L.stream);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

int check_image(orbx_ctx* c, const void* img, int w, int h, int stride) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!img) return fail(c, ORBX_ERR_INVALID_ARG, "image is NULL");
  if (w < 8 || h < 8 || w > c->p.max_width || h > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "image size outside [8, max_width] x [8, max_height]");
  if (stride < w) return fail(c, ORBX_ERR_INVALID_ARG, "stride < width");
  return ORBX_OK;
}

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
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

// separable kind -> register-streaming kernel; /273 kind -> LDS tile kernel (impl: see blur_impl_env)
hipError_t launch_blur_auto(int impl, hipStream_t s, const OrbxPlan& P, const OrbxTileMap& tm1, const OrbxTileDesc* tiles2,
                            int ntiles2, int n, const uint8_t* src, uint8_t* dst, int first_level, int kind) {
  if (kind == ORBX_BLUR_SEP16 && impl == 3)
    return orbx_launch_blur4(s, tiles2, ntiles2, P.frame_bytes, n, src, dst, first_level);
  if (kind == ORBX_BLUR_SEP16 && impl != 1)
    return orbx_launch_blur3(s, tiles2, ntiles2, P.frame_bytes, n, src, dst, first_level);
  return orbx_launch_blur(s, P, tm1, n, src, dst, first_level, kind);
}

int SideWork::wait(orbx_ctx* c) {
  if (ev) HIPCHK(c, hipEventSynchronize(ev));
  return ORBX_OK;
}

int SideWork::enter(orbx_ctx* c, hipStream_t s) {
  if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (stream != s) {
    const int st = wait(c);
    if (st != ORBX_OK) return st;
  }
  stream = s;
  return ORBX_OK;
}

int SideWork::after(orbx_ctx* c, const SideWork& producer, hipStream_t s) {
  if (producer.ev && producer.stream != s) HIPCHK(c, hipStreamWaitEvent(s, producer.ev, 0));
  return ORBX_OK;
}

int SideWork::grow(orbx_ctx* c, DevBuf& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return ORBX_OK;
  const int st = wait(c);
  if (st != ORBX_OK) return st;
  bytes = align_up_sz(std::max<size_t>(bytes, 256), 256);
  void* p = nullptr;
  HIPCHK(c, hipMalloc(&p, bytes));
  if (b.p) (void)hipFree(b.p);
  b.p = p;
  b.bytes = bytes;
  return ORBX_OK;
}

int PinnedUpload::send(orbx_ctx* c, void* d_dst, const void* src, size_t n, hipStream_t s) {
  if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(c, hipEventSynchronize(ev));  // the previous copy has to have read the mirror
  if (bytes < n) {
    if (host) (void)hipHostFree(host);
    host = nullptr;
    bytes = 0;
    HIPCHK(c, hipHostMalloc(&host, align_up_sz(n, 4096), hipHostMallocDefault));
    bytes = align_up_sz(n, 4096);
  }
  std::memcpy(host, src, n);
  HIPCHK(c, hipMemcpyAsync(d_dst, host, n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(ev, s));
  return ORBX_OK;
}

int set_workspace_limit(orbx_ctx* c, SideWork& side, std::initializer_list<DevBuf*> ws, size_t* limit, size_t bytes,
                        size_t dflt) {
  const int st = side.wait(c);
  if (st != ORBX_OK) return st;
  for (DevBuf* b : ws)
    if (b->p) {
      HIPCHK(c, hipFree(b->p));
      *b = DevBuf{};
    }
  *limit = bytes ? bytes : dflt;
  return ORBX_OK;
}

int stage_tracks(orbx_ctx* c, SideWork& side, DevBuf& stage, const float* tracks_xy, const int32_t* seen, int n_slots,
                 int window_len, const float** d_tracks, const int32_t** d_seen) {
  int st = side.enter(c, c->stream);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{side, c->stream};
  const size_t tb = sizeof(float) * 2 * (size_t)n_slots * window_len, sb = sizeof(int32_t) * (size_t)n_slots;
  const size_t o_seen = align_up_sz(tb, 256);
  if ((st = side.grow(c, stage, o_seen + sb)) != ORBX_OK) return st;
  uint8_t* d = (uint8_t*)stage.p;
  HIPCHK(c, hipMemcpyAsync(d, tracks_xy, tb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + o_seen, seen, sb, hipMemcpyHostToDevice, c->stream));
  *d_tracks = (const float*)d;
  *d_seen = (const int32_t*)(d + o_seen);
  return ORBX_OK;
}

int check_device_frames(orbx_ctx* c, const void* d_frames, int n, int n_min, int n_max, int w, int h, int row_stride,
                        size_t frame_stride, const FramesWhat& what) {
  if (!d_frames) return fail(c, ORBX_ERR_INVALID_ARG, what.null_msg);
  if (n < n_min || n > n_max) return fail(c, ORBX_ERR_INVALID_ARG, what.range_msg);
  if (w < 8 || h < 8 || w > c->p.max_width || h > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "image size outside [8, max_width] x [8, max_height]");
  if (row_stride < w) return fail(c, ORBX_ERR_INVALID_ARG, "row_stride < width");
  if (frame_stride < (size_t)row_stride * (size_t)(h - 1) + (size_t)w)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame_stride smaller than a frame");
  if ((unsigned long long)row_stride * (unsigned long long)(h - 1) + (unsigned long long)w > 0x7fffffffull)
    return fail(c, ORBX_ERR_INVALID_ARG, "row_stride * (height - 1) + width exceeds 2^31 - 1");
  return ORBX_OK;
}

}  // namespace orbx_host

namespace {

// ---- the environment switches ----
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

// ORBX_BLUR_IMPL (read when a context is created): 2 (default) k_blur3, 4 pixels per lane; 3: k_blur4, 16 pixels per
// lane (measured 9 % slower: the blur's vertical pass dominates its instruction count, and 94 registers leave 5
// waves per SIMD); 1: the first-generation LDS tile kernel.  The strip table is built for the kernel that reads it.
int blur_impl_env() {
  const int v = env_int("ORBX_BLUR_IMPL", 2);
  return v >= 1 && v <= 3 ? v : 2;
}

// ORBX_FAST_EARLY=0: every tile of FAST + NMS does the full work (results are identical).  Otherwise the tiles that
// provably cannot contribute to the first `cap` row-major survivors exit early (see decode_band in the kernels).
int fast_early_env() {
  static const int v = env_int("ORBX_FAST_EARLY", 1);
  return v;
}

// ORBX_FUSE=0: separate pyramid and blur kernels (same results; A/B timing and per-kernel profiles)
int fuse_env() {
  static const int v = env_int("ORBX_FUSE", 1);
  return v;
}

// ORBX_GRAPH=0: every batch is enqueued launch by launch, none replayed from a captured graph (run_batch)
int graph_env() {
  static const int v = env_int("ORBX_GRAPH", 1);
  return v;
}

// ORBX_SELECT_SPREAD=0/1 forces the fused / the three-kernel selection (A/B timing); frames whose candidates do not
// fit the fused kernel's LDS take the three kernels whatever it says (orbx_launch_level_select_auto)
int select_spread_env() {
  static const int v = env_int("ORBX_SELECT_SPREAD", -1);
  return v;
}

// ---- what the switches and the context's own settings add up to ----
bool fused_pyrblur(const orbx_ctx* c) {
  return fuse_env() && c->fuse && c->p.blur_levels == ORBX_BLUR_ALL && c->p.blur_kind == ORBX_BLUR_SEP16;
}
bool fast_early_on(const orbx_ctx* c) { return fast_early_env() && c->fast_early; }
bool blur_enabled(const orbx_ctx* c) { return c->p.blur_levels != ORBX_BLUR_NONE; }
const uint8_t* final_pyr(const orbx_ctx* c) { return blur_enabled(c) ? cur_lane(c).d_pyr_blur : cur_lane(c).d_pyr; }

// slots per frame of a result block written under plan P (nfeatures too small for any quota: one empty slot)
int slots_per_frame(const OrbxPlan& P) { return P.out_cap > 0 ? P.out_cap : 1; }

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

// the adaptive first pass (orbx_adapt.h) only where the top-rows-first pipeline can run at all
bool tile_prefs_apply(const orbx_ctx* c) {
  return c->adapt.top_mode == 2 && top_rows_env() > 0 && fast_early_on(c) && fused_pyrblur(c);
}
// what the scheduler's steps see of the context, and where its trace goes
OrbxAdaptGeom adapt_geom(const orbx_ctx* c) {
  return OrbxAdaptGeom{c->plan, c->bm_fast, c->p.nms_window / 2, c->fast_impl, top_rows_env()};
}
FILE* adapt_trace(const orbx_ctx* c) { return c->adapt.split_trace ? stderr : nullptr; }

// The tables of a frame size: built on the host (orbx_tables.h: the plan with its taps, then every table, each
// checked against its pool), then copied to the pools and committed.
int set_plan(orbx_ctx* c, int w, int h) {
  if (w == c->plan_w && h == c->plan_h) return ORBX_OK;
  if (w < 8 || h < 8 || w > c->p.max_width || h > c->p.max_height)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame size outside [8, max_width] x [8, max_height]");
  OrbxPlan plan;
  std::string why;
  int st = plan_with_taps(c->p, w, h, c->fast_impl, &plan, &c->h_taps, &why);
  if (st != ORBX_OK) return fail(c, st, why);
  if (c->h_taps.size() > c->table_cap.taps) return fail(c, ORBX_ERR_UNSUPPORTED, "resize table exceeds pool");
  // no plan is set until every table below is in place: a call that fails on the way must not leave the previous
  // size's (plan_w, plan_h) standing for tables that are half replaced
  c->plan_w = c->plan_h = 0;
  OrbxPlanTables& T = c->scratch;
  const OrbxTableSwitches sw{c->fast_impl, c->blur_impl, top_rows_env(), pyr_group_env() > 0, tile_prefs_apply(c)};
  st = build_tile_tables(plan, c->p.nms_window / 2, sw, c->table_cap, c->adapt, adapt_trace(c), &T, &why);
  if (st != ORBX_OK) return fail(c, st, why);
  // the tables may still be in use by an in-flight batch of the previous size
  HIPCHK(c, hipStreamSynchronize(batch_stream(c)));
  HIPCHK(c, lanes_sync(c));
  HIPCHK(c, hipMemcpy(c->d_taps, c->h_taps.data(), c->h_taps.size() * sizeof(OrbxResizeTap),
                      hipMemcpyHostToDevice));
  // the fused pyramid + blur kernel writes only the dwords that hold image pixels; consumers rely on the
  // padding bytes of a level being zero (BRIEF's zero-extension), and another frame size re-uses the pool
  // (both lanes' pools; on the context's stream, and waited for: batches may run on a caller's stream)
  for (const Lane& L : c->lanes)
    if (L.d_pyr_blur)
      HIPCHK(c, hipMemsetAsync(L.d_pyr_blur, 0, (size_t)c->p.max_batch * (size_t)c->plan_max.frame_bytes, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < kTileTables; i++) {
    const std::vector<OrbxTileDesc>& t = T.tiles[i];
    if (!t.empty())  // (no second pass / no FAST tile at all: nothing to copy)
      HIPCHK(c, hipMemcpy(c->tiles[i].d, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
    c->tiles[i].count = (int)t.size();
  }
  c->plan = plan;
  c->tm_blur = T.tm_blur;
  c->bm_fast = T.bm_fast;
  c->top_levels = T.top_levels;
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
  const bool two_pass = fused && !small && fast_early_on(c) && top_rows_wanted(c->adapt, top_rows_env()) && rest.count > 0 &&
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
  HIPCHK(c, orbx_launch_level_select_auto(s, P, n, c->p.select_mode, select_spread_env(), L.d_mask, final_pyr(c), c->d_gauss,
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
  // (h_feedback is never NULL in a context that orbx_create has returned: no guard here or at the verdict below)
  OrbxAdapt& a = c->adapt;
  if (w != a.learn_w || h != a.learn_h) {
    new_frame_size(a, w, h, const_cast<uint32_t*>(c->h_feedback));
  } else if (w == c->plan_w && h == c->plan_h) {
    bool any_pref = false;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) any_pref |= a.tile_h_pref[l] != 0 || a.cut_pref[l] != 0 || a.cut_force[l] != 0;
    // ONE snapshot of the pinned feedback words per batch, without waiting: whatever has arrived (orbx_adapt.h; the
    // words of the plan's levels, which lie in front: the cache lines the device has just written are the cost)
    const bool apply = tile_prefs_apply(c);
    const int used = ORBX_FEEDBACK_HIST + c->plan.nlevels * ORBX_FILL_BUCKETS;
    uint32_t words[ORBX_FEEDBACK_WORDS];
    for (int i = 0; apply && i < used; i++) words[i] = c->h_feedback[i];
    // (a switch that takes the top-rows-first pipeline away, or brings it back, since the tables were built)
    if (adapt_tile_rows(a, adapt_geom(c), words, apply, c->batch_serial, adapt_trace(c)) || (any_pref && apply != a.prefs_applied))
      c->plan_w = 0;
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
  top_rows_update(a, *reinterpret_cast<const volatile uint64_t*>(c->h_feedback));
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
  B.layout = OutLayout(n, B.cap);
  const int tm = c->timing;
  if (graph_env() && tm == 0) {
    const OrbxGraphKey key{d_frames, frame_stride, n, w, h, row_stride, (fast_early_on(c) ? 1 : 0) | (fused_pyrblur(c) ? 2 : 0) | (top_rows_wanted(a, top_rows_env()) ? 4 : 0) | (lanes ? 8 : 0) | (c->lane << 4) | (c->host_results ? 64 : 0),
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
  // every subsystem releases what it owns.  The landmarks before the windows tracker, the tracker before the good
  // features: each waits for its own event before its buffers go, and each may be reading the next one's block.
  c->carry.release();
  c->reloc.release();
  c->search.release();  // (its gated half ran under the re-association's event, waited for just above)
  c->pnp.release();
  c->st.release();
  c->wp.release();
  c->tp.release();
  c->lm.release();
  c->prior.release();  // (behind the landmarks' event, which its work ran under)
  c->lkw.release();
  c->gf.release();
  c->s.release();
  c->m.release();
  c->lk.release();
  c->pose.release();
  c->scale.release();
  c->ba.release();
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
  first_split_fields(c->adapt, getenv("ORBX_TOP_ROWS"));
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
  c->table_cap = tcap;
  for (int i = 0; i < kTileTables; i++)
    CREATE_CHK(hipMalloc((void**)&c->tiles[i].d, std::max<size_t>(tile_table_capacity(tcap, i), 1) * sizeof(OrbxTileDesc)));
  // (level sizes of smaller frames never exceed those of the largest frame)
  CREATE_CHK(hipMalloc((void**)&c->d_taps, tcap.taps * sizeof(OrbxResizeTap)));
  {
    const int K = p->harris_window;
    std::vector<float> g((size_t)K * K);
    gaussian_kernel(K, -1.0f, g.data());
    CREATE_CHK(hipMalloc((void**)&c->d_gauss, g.size() * sizeof(float)));
    CREATE_CHK(hipMemcpy(c->d_gauss, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  {
    const OutLayout o((int)B, slots_per_frame(M));  // (the largest block any batch can need)
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
  return run_batch(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride, stream_of(c, stream), true);
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

// Debug entry (tests): one level of one frame of the current lane's blurred pyramid, rows packed.
int orbx_debug_read_pyramid_level(orbx_ctx* c, int frame, int level, uint8_t* out, size_t out_bytes) {
  DeviceGuard _dg(c);
  if (!c || !out) return ORBX_ERR_INVALID_ARG;
  if (c->plan_w == 0 || !cur_lane(c).d_pyr_blur) return fail(c, ORBX_ERR_INVALID_ARG, "run a batch first");
  if (frame < 0 || frame >= c->p.max_batch || level < 0 || level >= c->plan.nlevels)
    return fail(c, ORBX_ERR_INVALID_ARG, "frame or level out of range");
  const OrbxLevel& V = c->plan.L[level];
  if (out_bytes < (size_t)V.w * (size_t)V.h) return fail(c, ORBX_ERR_INVALID_ARG, "out_bytes below level_w * level_h");
  if (c->last_stream) HIPCHK(c, hipStreamSynchronize(c->last_stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, lanes_sync(c));
  HIPCHK(c, hipMemcpy2D(out, (size_t)V.w, cur_lane(c).d_pyr_blur + (size_t)frame * (size_t)c->plan.frame_bytes + (size_t)V.img_off,
                        (size_t)V.pitch, (size_t)V.w, (size_t)V.h, hipMemcpyDeviceToHost));
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
  c->adapt.top_mode = mode;
  c->adapt.top_on = true;
  c->adapt.top_single_batches = 0;
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
      long long surv = 0, surv0 = 0;  // the kernel's tests: survivors of the first-pass tile rows, and of tile row 0
      for (int b = 0; b < std::min(top, c->bm_fast.tiles_y[l]); b++) {
        surv += (long long)(uint32_t)h[(size_t)f * ORBX_FAST_STAT_WORDS + (size_t)l * ORBX_MAX_BANDS + b];
        if (b == 0) surv0 = surv;
      }
      // (an early band, rows [early, first), is produced unless tile row 0 alone holds the cap)
      const int early_l = c->adapt.early_rows[l], early = early_l > 0 && early_l < first ? early_l : first;
      const int band = surv0 >= L.cap ? 0 : first - early;
      done += (long long)L.w * (first < L.h && surv >= L.cap ? early + band : L.h);
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

}  // extern "C"
