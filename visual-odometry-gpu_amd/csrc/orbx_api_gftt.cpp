// orbx_api_gftt.cpp -- host layer of liborbx.so (orbx_host.h): Shi-Tomasi corners (goodFeaturesToTrack).
#include <algorithm>
#include <cmath>

#include "orbx_host.h"

using namespace orbx_host;

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

// the workspace: allocated once, for as many frames of the largest size as the limit holds (at least one, at most
// max_batch)
int gf_workspace(orbx_ctx* c) {
  if (c->gf.ws.p) return ORBX_OK;
  const int mw = c->p.max_width, mh = c->p.max_height;
  const size_t one = gf_layout(1, mw, mh, gf_grid_bound(mw, mh)).total + 1024;
  const size_t frames = std::min<size_t>(std::max<size_t>(c->gf.ws_limit / one, 1), (size_t)c->p.max_batch);
  ENSURE(c, c->gf.ws, gf_layout((int)frames, mw, mh, gf_grid_bound(mw, mh)).total + 1024);
  return ORBX_OK;
}

// frames of w x h per slice
int gf_slice_frames(const orbx_ctx* c, int n, int w, int h, size_t grid_stride) {
  const size_t one = gf_layout(1, w, h, grid_stride).total + 1024;  // (the sections' alignment: < 1024 bytes)
  const size_t fit = std::max<size_t>((c->gf.ws.bytes - 1024) / one, 1);
  const int m = (int)std::min<size_t>(fit, (size_t)n);
  const int slices = (n + m - 1) / m;
  return (n + slices - 1) / slices;  // even slices
}

// enqueues the three stages for n device frames; the results go to gf.res (counts | corners)
int gf_run(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
           const GfArgs& a, hipStream_t s) {
  int st = c->gf.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->gf.side, s};
  c->gf.n = 0;  // (a failed call leaves no "last batch")
  if ((st = gf_workspace(c)) != ORBX_OK) return st;
  const size_t o_corners = align_up_sz(sizeof(int32_t) * (size_t)n, 256);
  const size_t res_bytes = o_corners + sizeof(float) * 2 * (size_t)a.cap * n;
  if (c->gf.res.p && c->gf.res.bytes < res_bytes && (st = c->gf.side.wait(c)) != ORBX_OK) return st;  // (still written?)
  ENSURE(c, c->gf.res, res_bytes);
  const size_t grid_stride = a.suppress ? (size_t)a.gw * a.gh * a.slots : 0;
  const int per = gf_slice_frames(c, n, w, h, grid_stride);
  int32_t* d_counts = (int32_t*)c->gf.res.p;
  float* d_corners = (float*)((uint8_t*)c->gf.res.p + o_corners);
  for (int f0 = 0; f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    const GfLayout L = gf_layout(m, w, h, grid_stride);
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
  ENSURE(c, c->gf.img, (size_t)w * h);
  HIPCHK(c, hipMemcpy2DAsync(c->gf.img.p, w, image, stride, w, h, hipMemcpyHostToDevice, c->stream));
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
  const GfLayout L = gf_layout(1, width, height, 0);
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
    HIPCHK(c, hipMemcpy(corners_xy, (const uint8_t*)c->gf.res.p + align_up_sz(sizeof(int32_t), 256),
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
                stream ? (hipStream_t)stream : c->stream);
}

int orbx_good_features_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return set_workspace_limit(c, c->gf.side, c->gf.ws, &c->gf.ws_limit, bytes, ORBX_GFTT_WORKSPACE_DEFAULT);
}

int orbx_good_features_results_device(orbx_ctx* c, orbx_good_features_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->gf.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  v->counts = (const int32_t*)c->gf.res.p;
  v->corners_xy = (const float*)((const uint8_t*)c->gf.res.p + align_up_sz(sizeof(int32_t) * (size_t)c->gf.n, 256));
  v->slot_capacity = c->gf.cap;
  v->n = c->gf.n;
  return ORBX_OK;
}

int orbx_good_features_fetch(orbx_ctx* c, int first, int n, int32_t* counts, float* corners_xy) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->gf.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no good-features batch has run");
  if (!counts || first < 0 || n < 1 || first >= c->gf.n || n > c->gf.n - first)
    return fail(c, ORBX_ERR_INVALID_ARG, "counts is NULL or [first, first + n) outside the batch");
  const int st = c->gf.side.wait(c);
  if (st != ORBX_OK) return st;
  const uint8_t* res = (const uint8_t*)c->gf.res.p;
  HIPCHK(c, hipMemcpy(counts, res + sizeof(int32_t) * (size_t)first, sizeof(int32_t) * (size_t)n,
                      hipMemcpyDeviceToHost));
  if (corners_xy) {
    const size_t row = sizeof(float) * 2 * (size_t)c->gf.cap;
    HIPCHK(c, hipMemcpy(corners_xy, res + align_up_sz(sizeof(int32_t) * (size_t)c->gf.n, 256) + row * first, row * n,
                        hipMemcpyDeviceToHost));
  }
  return ORBX_OK;
}

}  // extern "C"
