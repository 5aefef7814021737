// orbx_api_gftt.cpp -- host layer of liborbx.so (orbx_host.h): Shi-Tomasi corners (goodFeaturesToTrack), plain, with a
// mask, and topping up tracked points.
#include <algorithm>
#include <cmath>

#include "orbx_host.h"

using namespace orbx_host;

// ---- Shi-Tomasi corners (next row) ------------------------
namespace {

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

// the workspace: allocated once, for as many frames of the largest size as the limit holds; the bit maps of rank 12
// are allocated beside it at the first top-up or masked call, for the same number (orbx_layout.h)
int gf_frames(const orbx_ctx* c) {
  return (int)gf_workspace_frames(c->gf.ws_limit, c->p.max_width, c->p.max_height, c->p.max_batch);
}
int gf_workspace(orbx_ctx* c) {
  if (c->gf.ws.p) return ORBX_OK;
  return c->gf.side.grow(c, c->gf.ws, gf_workspace_bytes(gf_frames(c), c->p.max_width, c->p.max_height));
}
int gf_bitmaps(orbx_ctx* c) {
  if (c->gf.bm.p) return ORBX_OK;
  return c->gf.side.grow(c, c->gf.bm, gb_bytes(gf_frames(c), c->p.max_width, c->p.max_height));
}

// enqueues the three stages for n device frames; the results go to gf.res (counts | corners)
int gf_run(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
           const GfArgs& a, hipStream_t s) {
  int st = c->gf.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->gf.side, s};
  c->gf.n = 0;  // (a failed call leaves no "last batch")
  if ((st = gf_workspace(c)) != ORBX_OK) return st;
  const GrLayout R(n, a.cap);
  if ((st = c->gf.side.grow(c, c->gf.res, R.total)) != ORBX_OK) return st;
  const size_t grid_stride = a.suppress ? (size_t)a.gw * a.gh * a.slots : 0;
  const int per = gf_slice_frames(c->gf.ws.bytes, n, w, h, grid_stride);
  int32_t* d_counts = (int32_t*)c->gf.res.p;
  float* d_corners = (float*)((uint8_t*)c->gf.res.p + R.corners);
  for (int f0 = 0; f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    const GfLayout L(m, w, h, grid_stride);
    uint8_t* ws = (uint8_t*)c->gf.ws.p;
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
  c->gf.n = n;
  c->gf.cap = a.cap;
  return ORBX_OK;
}

// a host image, tightly packed, in gf.img on the context's stream
int gf_upload(orbx_ctx* c, const uint8_t* image, int w, int h, int stride) {
  int st = c->gf.side.enter(c, c->stream);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->gf.side, c->stream};
  if ((st = c->gf.side.grow(c, c->gf.img, (size_t)w * h)) != ORBX_OK) return st;
  HIPCHK(c, hipMemcpy2DAsync(c->gf.img.p, w, image, stride, w, h, hipMemcpyHostToDevice, c->stream));
  return ORBX_OK;
}

// ---- masked detection that tops up tracked points -----------------------
struct GfSeeds {  // d_xy == NULL: none
  const float* d_xy;
  size_t point_stride, frame_stride;
  const int32_t* d_seen;
  int seen_min, capacity;
};

// enqueues the stages for n device frames; blocked pixels come from the seeds or, for one frame, from d_mask (tight
// rows); the results go to gf.tres
int gf_topup_run(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
                 const GfSeeds& seeds, const uint8_t* d_mask, const GfArgs& a, int slot_cap, hipStream_t s) {
  int st = c->gf.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->gf.side, s};
  // the seeds may be the windows tracker's block, written on another stream
  if ((st = c->gf.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  c->gf.tn = 0;  // (a failed call leaves no "last top-up")
  if ((st = gf_workspace(c)) != ORBX_OK || (st = gf_bitmaps(c)) != ORBX_OK) return st;
  const GtLayout R(n, slot_cap);
  if ((st = c->gf.side.grow(c, c->gf.tres, R.total)) != ORBX_OK) return st;
  const size_t grid_stride = a.suppress ? (size_t)a.gw * a.gh * a.slots : 0;
  const int per = (int)std::min<size_t>((size_t)gf_slice_frames(c->gf.ws.bytes, n, w, h, grid_stride),
                                        gb_frames(c->gf.bm.bytes, w, h));
  uint8_t* res = (uint8_t*)c->gf.tres.p;
  int32_t* d_counts = (int32_t*)res;
  int32_t* d_carried = (int32_t*)(res + R.carried);
  float* d_points = (float*)(res + R.points);
  int32_t* d_origin = (int32_t*)(res + R.origin);
  const int max_seeds = std::min(seeds.d_xy ? seeds.capacity : 0, slot_cap);
  for (int f0 = 0; f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    const GfLayout L(m, w, h, grid_stride);
    const GbLayout B(m, w, h);
    uint8_t* ws = (uint8_t*)c->gf.ws.p;
    uint32_t* d_max = (uint32_t*)(ws + L.cnt);
    int32_t* d_ncand = (int32_t*)(d_max + m);
    uint32_t* d_mmax = (uint32_t*)c->gf.bm.p;
    uint32_t* d_bits = (uint32_t*)((uint8_t*)c->gf.bm.p + B.bits);
    float* pts = d_points + (size_t)2 * slot_cap * f0;
    HIPCHK(c, hipMemsetAsync(d_max, 0, 2 * sizeof(uint32_t) * (size_t)m, s));
    HIPCHK(c, hipMemsetAsync(d_mmax, 0, sizeof(uint32_t) * (size_t)m, s));
    if (a.suppress) HIPCHK(c, hipMemsetAsync(ws + L.grid, 0xff, sizeof(uint32_t) * grid_stride * m, s));
    HIPCHK(c, orbx_launch_gftt_seeds(s, m, seeds.d_xy ? seeds.d_xy + seeds.frame_stride * (size_t)f0 : nullptr,
                                     seeds.point_stride, seeds.frame_stride,
                                     seeds.d_seen ? seeds.d_seen + (size_t)seeds.capacity * f0 : nullptr,
                                     seeds.seen_min, seeds.capacity, w, h, slot_cap, d_carried + f0, pts,
                                     d_origin + (size_t)slot_cap * f0));
    if (d_mask) {
      HIPCHK(c, orbx_launch_gftt_mask_bits(s, d_mask, w, h, w, d_bits));
    } else {
      HIPCHK(c, hipMemsetAsync(d_bits, 0, sizeof(uint32_t) * B.words * m, s));
      if (a.suppress && max_seeds > 0)
        HIPCHK(c, orbx_launch_gftt_block(s, m, pts, d_carried + f0, slot_cap, max_seeds, w, h, a.min_distance, d_bits));
    }
    HIPCHK(c, orbx_launch_gftt_response(s, d_frames + frame_stride * (size_t)f0, m, w, h, row_stride, frame_stride,
                                        (float*)(ws + L.map), d_max));
    HIPCHK(c, orbx_launch_gftt_masked_max(s, (const float*)(ws + L.map), m, w, h, d_bits, d_mmax));
    HIPCHK(c, orbx_launch_gftt_candidates_blocked(s, (const float*)(ws + L.map), m, w, h, d_mmax, a.quality,
                                                  (unsigned long long*)(ws + L.keys), L.pool, d_ncand, d_bits));
    HIPCHK(c, orbx_launch_gftt_select_topup(s, m, w, (unsigned long long*)(ws + L.keys), L.pool, d_ncand,
                                            a.min_distance, a.cell, a.gw, a.gh, a.slots, (uint32_t*)(ws + L.grid),
                                            grid_stride, slot_cap, d_carried + f0, d_counts + f0, pts));
  }
  c->gf.tn = n;
  c->gf.tcap = slot_cap;
  return ORBX_OK;
}

int gf_check_topup_params(orbx_ctx* c, double quality, double min_distance) {
  const int st = gf_check_params(c, quality, min_distance);
  if (st != ORBX_OK) return st;
  if (min_distance > ORBX_GFTT_TOPUP_MAX_MIN_DISTANCE)
    return fail(c, ORBX_ERR_UNSUPPORTED, "min_distance above ORBX_GFTT_TOPUP_MAX_MIN_DISTANCE");
  return ORBX_OK;
}

// host memory (`rows` rows of `row` bytes, src_stride apart) packed tightly into gf.stage on the context's stream:
// the seeds or the mask of the one-frame entries
int gf_stage(orbx_ctx* c, const void* src, size_t row, size_t rows, size_t src_stride) {
  int st = c->gf.side.enter(c, c->stream);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->gf.side, c->stream};
  if ((st = c->gf.side.grow(c, c->gf.stage, row * rows)) != ORBX_OK) return st;
  HIPCHK(c, hipMemcpy2DAsync(c->gf.stage.p, row, src, src_stride, row, rows, hipMemcpyHostToDevice, c->stream));
  return ORBX_OK;
}

// the one-frame result of the run just enqueued on the context's stream, to host arrays of `capacity` slots
int gf_topup_deliver(orbx_ctx* c, float* points_xy, int32_t* origin, int capacity, int* count, int* carried) {
  const GtLayout R(1, c->gf.tcap);
  const uint8_t* res = (const uint8_t*)c->gf.tres.p;
  int32_t found = 0, kept = 0;
  HIPCHK(c, hipMemcpyAsync(&found, res, sizeof(found), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&kept, res + R.carried, sizeof(kept), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (found > capacity) {
    *count = found;
    return fail(c, ORBX_ERR_CAPACITY, "the result arrays are too small");
  }
  if (found > 0) {
    HIPCHK(c, hipMemcpy(points_xy, res + R.points, sizeof(float) * 2 * (size_t)found, hipMemcpyDeviceToHost));
    if (origin) HIPCHK(c, hipMemcpy(origin, res + R.origin, sizeof(int32_t) * (size_t)found, hipMemcpyDeviceToHost));
  }
  *count = found;
  if (carried) *carried = kept;
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
  const SideWork::Mark mark{c->gf.side, c->stream};
  if ((st = gf_workspace(c)) != ORBX_OK) return st;
  const GfLayout L(1, width, height, 0);
  uint8_t* ws = (uint8_t*)c->gf.ws.p;
  HIPCHK(c, hipMemsetAsync(ws + L.cnt, 0, 2 * sizeof(uint32_t), c->stream));
  HIPCHK(c, orbx_launch_gftt_response(c->stream, (const uint8_t*)c->gf.img.p, 1, width, height, width,
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
  if ((st = gf_run(c, (const uint8_t*)c->gf.img.p, 1, width, height, width, (size_t)width * height, a, c->stream)) !=
      ORBX_OK)
    return st;
  int32_t found = 0;
  HIPCHK(c, hipMemcpyAsync(&found, c->gf.res.p, sizeof(found), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (found > capacity) {
    *count = found;
    return fail(c, ORBX_ERR_CAPACITY, "corners_xy is too small");
  }
  if (found > 0)
    HIPCHK(c, hipMemcpy(corners_xy, (const uint8_t*)c->gf.res.p + GrLayout(1, c->gf.cap).corners,
                        sizeof(float) * 2 * (size_t)found, hipMemcpyDeviceToHost));
  *count = found;
  return ORBX_OK;
}

int orbx_good_features_batch_device(orbx_ctx* c, const void* d_frames, int n, int width, int height, int row_stride,
                                    size_t frame_stride, int max_corners, double quality_level, double min_distance,
                                    void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = check_device_frames(c, d_frames, n, 1, c->p.max_batch, width, height, row_stride, frame_stride,
                               {"d_frames is NULL", "n outside [1, max_batch]"});
  if (st != ORBX_OK) return st;
  if (max_corners < 1) return fail(c, ORBX_ERR_INVALID_ARG, "max_corners < 1");
  if ((st = gf_check_params(c, quality_level, min_distance)) != ORBX_OK) return st;
  return gf_run(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride,
                gf_args(width, height, max_corners, quality_level, min_distance),
                stream_of(c, stream));
}

int orbx_good_features_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  // (the bit maps go with the workspace)
  return set_workspace_limit(c, c->gf.side, {&c->gf.ws, &c->gf.bm}, &c->gf.ws_limit, bytes, ORBX_GFTT_WORKSPACE_DEFAULT);
}

int orbx_good_features_results_device(orbx_ctx* c, orbx_good_features_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->gf.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  v->counts = (const int32_t*)c->gf.res.p;
  v->corners_xy = (const float*)((const uint8_t*)c->gf.res.p + GrLayout(c->gf.n, c->gf.cap).corners);
  v->slot_capacity = c->gf.cap;
  v->n = c->gf.n;
  return ORBX_OK;
}

int orbx_good_features_fetch(orbx_ctx* c, int first, int n, int32_t* counts, float* corners_xy) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->gf.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  if (!counts || !range_ok(first, n, c->gf.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "counts is NULL or [first, first + n) outside the batch");
  const int st = c->gf.side.wait(c);
  if (st != ORBX_OK) return st;
  const uint8_t* res = (const uint8_t*)c->gf.res.p;
  HIPCHK(c, hipMemcpy(counts, res + sizeof(int32_t) * (size_t)first, sizeof(int32_t) * (size_t)n,
                      hipMemcpyDeviceToHost));
  if (corners_xy) {
    const size_t row = sizeof(float) * 2 * (size_t)c->gf.cap;
    HIPCHK(c, hipMemcpy(corners_xy, res + GrLayout(c->gf.n, c->gf.cap).corners + row * first, row * n,
                        hipMemcpyDeviceToHost));
  }
  return ORBX_OK;
}

int orbx_good_features_topup_device(orbx_ctx* c, const void* d_frames, int n, int width, int height, int row_stride,
                                    size_t frame_stride, const float* d_seed_xy, size_t seed_point_stride,
                                    size_t seed_frame_stride, const int32_t* d_seed_seen, int seen_min,
                                    int seed_capacity, int max_corners, double quality_level, double min_distance,
                                    void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = check_device_frames(c, d_frames, n, 1, c->p.max_batch, width, height, row_stride, frame_stride,
                               {"d_frames is NULL", "n outside [1, max_batch]"});
  if (st != ORBX_OK) return st;
  if (max_corners < 1) return fail(c, ORBX_ERR_INVALID_ARG, "max_corners < 1");
  if (!d_seed_xy || seed_capacity < 1) return fail(c, ORBX_ERR_INVALID_ARG, "d_seed_xy is NULL or seed_capacity < 1");
  if (((uintptr_t)d_seed_xy | (uintptr_t)d_seed_seen) & 3u)
    return fail(c, ORBX_ERR_INVALID_ARG, "d_seed_xy / d_seed_seen is not 4-byte aligned");
  if (seed_point_stride < 2 || seed_point_stride > ((size_t)1 << 40) || seed_frame_stride > ((size_t)1 << 48) ||
      seed_frame_stride < seed_point_stride * (size_t)(seed_capacity - 1) + 2)
    return fail(c, ORBX_ERR_INVALID_ARG, "seed strides too small for seed_capacity slots of two floats");
  if ((st = gf_check_topup_params(c, quality_level, min_distance)) != ORBX_OK) return st;
  const uint8_t* lo = (const uint8_t*)c->gf.tres.p;
  if (lo && (const uint8_t*)d_seed_xy >= lo && (const uint8_t*)d_seed_xy < lo + c->gf.tres.bytes)
    return fail(c, ORBX_ERR_INVALID_ARG, "d_seed_xy lies inside the top-up's own result block");
  const GfSeeds seeds{d_seed_xy, seed_point_stride, seed_frame_stride, d_seed_seen, seen_min, seed_capacity};
  return gf_topup_run(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride, seeds, nullptr,
                      gf_args(width, height, max_corners, quality_level, min_distance), max_corners,
                      stream_of(c, stream));
}

int orbx_good_features_topup_results_device(orbx_ctx* c, orbx_good_features_topup_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->gf.tn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no top-up has run");
  const GtLayout R(c->gf.tn, c->gf.tcap);
  const uint8_t* res = (const uint8_t*)c->gf.tres.p;
  v->counts = (const int32_t*)res;
  v->carried = (const int32_t*)(res + R.carried);
  v->points_xy = (const float*)(res + R.points);
  v->origin = (const int32_t*)(res + R.origin);
  v->slot_capacity = c->gf.tcap;
  v->n = c->gf.tn;
  return ORBX_OK;
}

int orbx_good_features_topup_fetch(orbx_ctx* c, int first, int n, int32_t* counts, int32_t* carried, float* points_xy,
                                   int32_t* origin) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->gf.tn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no top-up has run");
  if (!counts || !range_ok(first, n, c->gf.tn))
    return fail(c, ORBX_ERR_INVALID_ARG, "counts is NULL or [first, first + n) outside the batch");
  const int st = c->gf.side.wait(c);
  if (st != ORBX_OK) return st;
  const GtLayout R(c->gf.tn, c->gf.tcap);
  const uint8_t* res = (const uint8_t*)c->gf.tres.p;
  const size_t cnt = sizeof(int32_t) * (size_t)n, slots = (size_t)c->gf.tcap;
  HIPCHK(c, hipMemcpy(counts, res + sizeof(int32_t) * (size_t)first, cnt, hipMemcpyDeviceToHost));
  if (carried)
    HIPCHK(c, hipMemcpy(carried, res + R.carried + sizeof(int32_t) * (size_t)first, cnt, hipMemcpyDeviceToHost));
  if (points_xy)
    HIPCHK(c, hipMemcpy(points_xy, res + R.points + sizeof(float) * 2 * slots * first, sizeof(float) * 2 * slots * n,
                        hipMemcpyDeviceToHost));
  if (origin)
    HIPCHK(c, hipMemcpy(origin, res + R.origin + sizeof(int32_t) * slots * first, sizeof(int32_t) * slots * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_good_features_topup(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                             const float* seeds_xy, int n_seeds, int max_corners, double quality_level,
                             double min_distance, float* points_xy, int32_t* origin, int capacity, int* count,
                             int* carried) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!count || !carried || capacity < 0 || (capacity > 0 && (!points_xy || !origin)))
    return fail(c, ORBX_ERR_INVALID_ARG, "count / carried / points_xy / origin is NULL or capacity < 0");
  if (n_seeds < 0 || (n_seeds > 0 && !seeds_xy)) return fail(c, ORBX_ERR_INVALID_ARG, "n_seeds < 0 or seeds_xy is NULL");
  if (max_corners < 1) return fail(c, ORBX_ERR_INVALID_ARG, "max_corners < 1");
  if ((st = gf_check_topup_params(c, quality_level, min_distance)) != ORBX_OK) return st;
  if ((st = gf_upload(c, image, width, height, stride)) != ORBX_OK) return st;
  if (n_seeds > 0 && (st = gf_stage(c, seeds_xy, sizeof(float) * 2 * (size_t)n_seeds, 1, sizeof(float) * 2 * (size_t)n_seeds)) != ORBX_OK) return st;
  const GfSeeds seeds{n_seeds > 0 ? (const float*)c->gf.stage.p : nullptr, 2, 2 * (size_t)n_seeds, nullptr, 0, n_seeds};
  if ((st = gf_topup_run(c, (const uint8_t*)c->gf.img.p, 1, width, height, width, (size_t)width * height, seeds,
                         nullptr, gf_args(width, height, max_corners, quality_level, min_distance), max_corners,
                         c->stream)) != ORBX_OK)
    return st;
  return gf_topup_deliver(c, points_xy, origin, capacity, count, carried);
}

int orbx_good_features_to_track_masked(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                                       const uint8_t* mask, int mask_stride, int max_corners, double quality_level,
                                       double min_distance, float* corners_xy, int capacity, int* count) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!mask || mask_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "mask is NULL or mask_stride < width");
  if (!count || capacity < 0 || (capacity > 0 && !corners_xy))
    return fail(c, ORBX_ERR_INVALID_ARG, "count / corners_xy is NULL or capacity < 0");
  if ((st = gf_check_topup_params(c, quality_level, min_distance)) != ORBX_OK) return st;
  if ((st = gf_upload(c, image, width, height, stride)) != ORBX_OK) return st;
  if ((st = gf_stage(c, mask, (size_t)width, (size_t)height, (size_t)mask_stride)) != ORBX_OK) return st;
  const GfArgs a = gf_args(width, height, max_corners, quality_level, min_distance);  // a.cap: the limit, or the pool
  const GfSeeds none{nullptr, 2, 0, nullptr, 0, 0};
  if ((st = gf_topup_run(c, (const uint8_t*)c->gf.img.p, 1, width, height, width, (size_t)width * height, none,
                         (const uint8_t*)c->gf.stage.p, a, a.cap, c->stream)) != ORBX_OK)
    return st;
  return gf_topup_deliver(c, corners_xy, nullptr, capacity, count, nullptr);
}

}  // extern "C"
