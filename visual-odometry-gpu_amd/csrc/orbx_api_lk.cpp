// orbx_api_lk.cpp -- host layer of liborbx.so (orbx_host.h): pyramidal Lucas-Kanade tracking, per pair of host
// images and over windows of device-resident frames.
#include <algorithm>
#include <cstring>

#include "orbx_host.h"

using namespace orbx_host;

// ---- pyramidal Lucas-Kanade tracking (src/feature_tracking.cpp:166-193) ------------------

namespace {
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
  const LkGeom g(width, height, win_size, max_level);
  int st;
  int ip;  // buffer holding the `prev` pyramid
  if (prev) {
    ip = c->lk.last == 0 ? 1 : 0;
    if ((st = lk_upload(c, g, c->lk.img[ip], prev, prev_stride)) != ORBX_OK) return st;
  } else {
    // the previous call's `next` image is this call's `prev` (img1 = img2.clone(), feature_tracking.cpp:112)
    if (c->lk.last < 0 || c->lk.w != width || c->lk.h != height || c->lk.top != g.top || c->lk.win != win_size)
      return fail(c, ORBX_ERR_INVALID_ARG, "prev == NULL needs a previous orbx_lk_track call of the same geometry");
    ip = c->lk.last;
  }
  const int in = 1 - ip;
  c->lk.last = -1;  // invalid until this call has succeeded
  if ((st = lk_upload(c, g, c->lk.img[in], next, next_stride)) != ORBX_OK) return st;
  ENSURE(c, c->lk.deriv, g.der_bytes + 256);
  const uint8_t* pimg = (const uint8_t*)c->lk.img[ip].p;
  for (int l = 0; l <= g.top; l++)
    HIPCHK(c, orbx_launch_lk_scharr(c->stream, pimg + g.img_off[l], g.w[l], g.h[l], g.pitch[l],
                                    reinterpret_cast<int16_t*>((uint8_t*)c->lk.deriv.p + g.der_off[l])));
  uint8_t* hio = nullptr;
  const LkIo L(n);
  if (n > 0) {
    DevBuf& io = c->lk.io;
    ENSURE(c, io, L.bytes);
    if (c->lk.host_bytes < L.bytes) {  // pinned staging: small pageable copies cost ~15 us each
      if (c->lk.host) (void)hipHostFree(c->lk.host);
      c->lk.host = nullptr;
      c->lk.host_bytes = 0;
      HIPCHK(c, hipHostMalloc(&c->lk.host, align_up_sz(L.bytes, 4096), hipHostMallocDefault));
      c->lk.host_bytes = align_up_sz(L.bytes, 4096);
    }
    hio = (uint8_t*)c->lk.host;
    std::memcpy(hio, prev_pts_xy, L.next);
    HIPCHK(c, hipMemcpyAsync(io.p, hio, L.next, hipMemcpyHostToDevice, c->stream));
    const OrbxLkPyr P = lk_pyr(g, pimg, (const uint8_t*)c->lk.deriv.p);
    const OrbxLkPyr N = lk_pyr(g, (const uint8_t*)c->lk.img[in].p, nullptr);
    HIPCHK(c, orbx_launch_lk_track(c->stream, P, N, n, at<float>(io, 0), at<float>(io, L.next), at<uint8_t>(io, L.status),
                                   at<float>(io, L.err), win_size, max_iters, epsilon * epsilon));
    // next points | err | status come back in one copy
    HIPCHK(c, hipMemcpyAsync(hio + L.next, at<uint8_t>(io, L.next), L.bytes - L.next, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n > 0) {
    std::memcpy(next_pts_xy, hio + L.next, L.next);
    std::memcpy(status, hio + L.status, (size_t)n);
    if (err) std::memcpy(err, hio + L.err, sizeof(float) * (size_t)n);
  }
  c->lk.w = width;
  c->lk.h = height;
  c->lk.top = g.top;
  c->lk.win = win_size;
  c->lk.last = in;
  return ORBX_OK;
}

int orbx_lk_pyramid_levels(int width, int height, int win_size, int max_level) {
  if (width < 1 || height < 1 || win_size < 3 || win_size > 31 || max_level < 0 || max_level >= ORBX_LK_MAX_LEVELS)
    return -1;
  return LkGeom(width, height, win_size, max_level).top + 1;
}

}  // extern "C"

// ---- Lucas-Kanade over frame windows ---------------------------------------------------------
// trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) for many windows per launch; with windows of two
// frames, track_optical_flow (src/feature_tracking.cpp:166-193) over a stream.  The entries with the
// forward-backward check (rank 13) are the same calls with a threshold: one lkw_run, one result block.

namespace {

FramesWhat lkw_frames_what(int max_frames) {
  return {"frames is NULL", "n_frames outside [2, " + std::to_string(max_frames) + "]"};
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

// fb_threshold of the entries with the forward-backward check (rank 13 rule 6): +inf and 0 are legal
int lkw_check_fb(orbx_ctx* c, float fb_threshold) {
  if (!(fb_threshold >= 0.f)) return fail(c, ORBX_ERR_INVALID_ARG, "fb_threshold is NaN or negative");
  return ORBX_OK;
}

// enqueues the pyramids and the tracking of every window on s; arguments are checked.  fb_threshold: NULL for the
// plain tracker, else the threshold of the forward-backward check (rank 13)
int lkw_run(orbx_ctx* c, const uint8_t* d_frames, int n_frames, int w, int h, int row_stride, size_t frame_stride,
            const int32_t* window_first, int n_windows, int window_len, const float* d_points,
            const int32_t* d_counts, int cap, int win, int max_level, int max_iters, double epsilon,
            const float* fb_threshold, hipStream_t s) {
  int st = c->lkw.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->lkw.side, s};
  // points and counts may be the good-features block, written on another stream
  if ((st = c->lkw.side.after(c, c->gf.side, s)) != ORBX_OK) return st;
  const LkwLayout L(w, h, win, max_level);
  const size_t fit = lkw_fit(c->lkw.ws_limit, L, window_len, n_frames);  // frames per slice
  const LkwResult R(n_windows, cap, window_len);
  const LkwFbResult FB(n_windows, cap, window_len);
  const size_t table = sizeof(int32_t) * (size_t)n_windows;
  if ((st = c->lkw.side.grow(c, c->lkw.ws, lkw_workspace_bytes(L, fit))) != ORBX_OK) return st;
  if ((st = c->lkw.side.grow(c, c->lkw.first, table)) != ORBX_OK) return st;
  if ((st = c->lkw.side.grow(c, c->lkw.res, R.bytes)) != ORBX_OK) return st;
  if (fb_threshold && (st = c->lkw.side.grow(c, c->lkw.fbres, FB.bytes)) != ORBX_OK) return st;
  // from here on the previous result is being replaced (a larger block has already taken its place)
  c->lkw.n = 0;
  if ((st = c->lkw.first_up.send(c, c->lkw.first.p, window_first, table, s)) != ORBX_OK) return st;
  uint8_t* ws = (uint8_t*)c->lkw.ws.p;
  uint8_t* res = (uint8_t*)c->lkw.res.p;
  uint8_t* fbres = (uint8_t*)c->lkw.fbres.p;
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
    uint8_t* ws_der = ws + lkw_der_offset(L, m);         // [m][levels 0 .. top]
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
    const int32_t* d_first = (const int32_t*)c->lkw.first.p + w0;
    const float* pts = d_points + 2 * slot_stride * w0;
    const int32_t* cnt = d_counts ? d_counts + w0 : nullptr;
    float* trk = (float*)res + 2 * slot_stride * window_len * w0;
    int32_t* seen = (int32_t*)(res + R.o_seen) + slot_stride * w0;
    float* err = (float*)(res + R.o_err) + slot_stride * (window_len - 1) * w0;
    if (fb_threshold)
      HIPCHK(c, orbx_launch_lk_track_windows_fb(s, F, d_first, w1 - w0, window_len, pts, cnt, cap, trk, seen, err,
                                                (float*)fbres + slot_stride * (window_len - 1) * w0,
                                                (int32_t*)(fbres + FB.o_lost) + slot_stride * w0, win, max_iters,
                                                epsilon * epsilon, (double)*fb_threshold * (double)*fb_threshold));
    else
      HIPCHK(c, orbx_launch_lk_track_windows(s, F, d_first, w1 - w0, window_len, pts, cnt, cap, trk, seen, err, win,
                                             max_iters, epsilon * epsilon));
    w0 = w1;
  }
  c->lkw.fb = fb_threshold != nullptr;
  c->lkw.n = n_windows;
  c->lkw.cap = cap;
  c->lkw.len = window_len;
  return ORBX_OK;
}

// behind orbx_lk_track_windows_device and its twin with the forward-backward check (fb_threshold != NULL)
int lkw_windows_device(orbx_ctx* c, const void* d_frames, int n_frames, int width, int height, int row_stride,
                       size_t frame_stride, const int32_t* window_first, int n_windows, int window_len,
                       const float* d_points_xy, const int32_t* d_counts, int slot_capacity, int win_size,
                       int max_level, int max_iters, double epsilon, const float* fb_threshold, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = check_device_frames(c, d_frames, n_frames, 2, c->p.max_batch, width, height, row_stride, frame_stride,
                               lkw_frames_what(c->p.max_batch));
  if (st != ORBX_OK) return st;
  if ((st = lkw_check_params(c, win_size, max_level, &max_iters, &epsilon)) != ORBX_OK) return st;
  if (fb_threshold && (st = lkw_check_fb(c, *fb_threshold)) != ORBX_OK) return st;
  if (!window_first || !d_points_xy) return fail(c, ORBX_ERR_INVALID_ARG, "window_first / d_points_xy is NULL");
  if (n_windows < 1 || window_len < 2 || slot_capacity < 1)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1, window_len < 2 or slot_capacity < 1");
  for (int i = 0; i < n_windows; i++)
    if (window_first[i] < 0 || window_first[i] > n_frames - window_len)
      return fail(c, ORBX_ERR_INVALID_ARG, "a window does not lie inside the frames");
  return lkw_run(c, (const uint8_t*)d_frames, n_frames, width, height, row_stride, frame_stride, window_first,
                 n_windows, window_len, d_points_xy, d_counts, slot_capacity, win_size, max_level, max_iters, epsilon,
                 fb_threshold, stream_of(c, stream));
}

}  // namespace

extern "C" {

int orbx_lk_track_windows_device(orbx_ctx* c, const void* d_frames, int n_frames, int width, int height,
                                 int row_stride, size_t frame_stride, const int32_t* window_first, int n_windows,
                                 int window_len, const float* d_points_xy, const int32_t* d_counts, int slot_capacity,
                                 int win_size, int max_level, int max_iters, double epsilon, void* stream) {
  return lkw_windows_device(c, d_frames, n_frames, width, height, row_stride, frame_stride, window_first, n_windows,
                            window_len, d_points_xy, d_counts, slot_capacity, win_size, max_level, max_iters, epsilon,
                            nullptr, stream);
}

int orbx_lk_track_windows_fb_device(orbx_ctx* c, const void* d_frames, int n_frames, int width, int height,
                                    int row_stride, size_t frame_stride, const int32_t* window_first, int n_windows,
                                    int window_len, const float* d_points_xy, const int32_t* d_counts,
                                    int slot_capacity, int win_size, int max_level, int max_iters, double epsilon,
                                    float fb_threshold, void* stream) {
  return lkw_windows_device(c, d_frames, n_frames, width, height, row_stride, frame_stride, window_first, n_windows,
                            window_len, d_points_xy, d_counts, slot_capacity, win_size, max_level, max_iters, epsilon,
                            &fb_threshold, stream);
}

int orbx_lk_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return set_workspace_limit(c, c->lkw.side, {&c->lkw.ws}, &c->lkw.ws_limit, bytes, ORBX_LK_WORKSPACE_DEFAULT);
}

int orbx_lk_windows_results_device(orbx_ctx* c, orbx_lk_windows_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->lkw.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  const LkwResult R(c->lkw.n, c->lkw.cap, c->lkw.len);
  const uint8_t* res = (const uint8_t*)c->lkw.res.p;
  v->tracks_xy = (const float*)res;
  v->seen = (const int32_t*)(res + R.o_seen);
  v->err = (const float*)(res + R.o_err);
  v->slot_capacity = c->lkw.cap;
  v->window_len = c->lkw.len;
  v->n_windows = c->lkw.n;
  return ORBX_OK;
}

int orbx_lk_windows_fetch(orbx_ctx* c, int first, int n, float* tracks_xy, int32_t* seen, float* err) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->lkw.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  if (!range_ok(first, n, c->lkw.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the batch");
  const int st = c->lkw.side.wait(c);
  if (st != ORBX_OK) return st;
  const LkwResult R(c->lkw.n, c->lkw.cap, c->lkw.len);
  const uint8_t* res = (const uint8_t*)c->lkw.res.p;
  const size_t slots = (size_t)c->lkw.cap, len = (size_t)c->lkw.len;
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

int orbx_lk_windows_fb_results_device(orbx_ctx* c, orbx_lk_windows_fb_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->lkw.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  if (!c->lkw.fb) return fail(c, ORBX_ERR_INVALID_ARG, "the last windows call had no forward-backward check");
  const LkwFbResult FB(c->lkw.n, c->lkw.cap, c->lkw.len);
  const uint8_t* fbres = (const uint8_t*)c->lkw.fbres.p;
  v->fb_d2 = (const float*)fbres;
  v->lost = (const int32_t*)(fbres + FB.o_lost);
  v->slot_capacity = c->lkw.cap;
  v->window_len = c->lkw.len;
  v->n_windows = c->lkw.n;
  return ORBX_OK;
}

int orbx_lk_windows_fb_fetch(orbx_ctx* c, int first, int n, float* fb_d2, int32_t* lost) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->lkw.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no LK windows batch has run");
  if (!c->lkw.fb) return fail(c, ORBX_ERR_INVALID_ARG, "the last windows call had no forward-backward check");
  if (!range_ok(first, n, c->lkw.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the batch");
  const int st = c->lkw.side.wait(c);
  if (st != ORBX_OK) return st;
  const LkwFbResult FB(c->lkw.n, c->lkw.cap, c->lkw.len);
  const uint8_t* fbres = (const uint8_t*)c->lkw.fbres.p;
  const size_t slots = (size_t)c->lkw.cap, len = (size_t)c->lkw.len;
  if (fb_d2)
    HIPCHK(c, hipMemcpy(fb_d2, fbres + sizeof(float) * slots * (len - 1) * first, sizeof(float) * slots * (len - 1) * n,
                        hipMemcpyDeviceToHost));
  if (lost)
    HIPCHK(c, hipMemcpy(lost, fbres + FB.o_lost + sizeof(int32_t) * slots * first, sizeof(int32_t) * slots * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

}  // extern "C"

namespace {

// behind orbx_lk_track_window and its twin with the forward-backward check (fb_threshold != NULL)
int lkw_window_host(orbx_ctx* c, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                    size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen, float* err,
                    int win_size, int max_level, int max_iters, double epsilon, const float* fb_threshold, float* fb_d2,
                    int32_t* lost) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  // (the host entry stages into a buffer of its own; 65535: blockIdx.z)
  int st = check_device_frames(c, frames, n_frames, 2, 65535, width, height, row_stride, frame_stride,
                               lkw_frames_what(65535));
  if (st != ORBX_OK) return st;
  if ((st = lkw_check_params(c, win_size, max_level, &max_iters, &epsilon)) != ORBX_OK) return st;
  if (fb_threshold && (st = lkw_check_fb(c, *fb_threshold)) != ORBX_OK) return st;
  if (n < 0 || (n > 0 && (!pts_xy || !tracks_xy || !seen)))
    return fail(c, ORBX_ERR_INVALID_ARG, "n < 0 or pts_xy / tracks_xy / seen is NULL");
  if (n == 0) return ORBX_OK;  // no points: nothing to track, the last result stays
  if ((st = c->lkw.side.enter(c, c->stream)) != ORBX_OK) return st;
  const size_t tight = (size_t)width * height;
  {
    const SideWork::Mark mark{c->lkw.side, c->stream};
    if ((st = c->lkw.side.grow(c, c->lkw.img, tight * n_frames)) != ORBX_OK) return st;
    if ((st = c->lkw.side.grow(c, c->lkw.pts, sizeof(float) * 2 * (size_t)n)) != ORBX_OK) return st;
    if (row_stride == width && frame_stride == tight) {
      HIPCHK(c, hipMemcpyAsync(c->lkw.img.p, frames, tight * n_frames, hipMemcpyHostToDevice, c->stream));
    } else {
      for (int i = 0; i < n_frames; i++)
        HIPCHK(c, hipMemcpy2DAsync((uint8_t*)c->lkw.img.p + tight * i, width, frames + frame_stride * i, row_stride,
                                   width, height, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->lkw.pts.p, pts_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  const int32_t first = 0;
  if ((st = lkw_run(c, (const uint8_t*)c->lkw.img.p, n_frames, width, height, width, tight, &first, 1, n_frames,
                    (const float*)c->lkw.pts.p, nullptr, n, win_size, max_level, max_iters, epsilon, fb_threshold,
                    c->stream)) != ORBX_OK)
    return st;
  if ((st = orbx_lk_windows_fetch(c, 0, 1, tracks_xy, seen, err)) != ORBX_OK) return st;
  return fb_threshold ? orbx_lk_windows_fb_fetch(c, 0, 1, fb_d2, lost) : ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_lk_track_window(orbx_ctx* c, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                         size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen, float* err,
                         int win_size, int max_level, int max_iters, double epsilon) {
  return lkw_window_host(c, frames, n_frames, width, height, row_stride, frame_stride, pts_xy, n, tracks_xy, seen, err,
                         win_size, max_level, max_iters, epsilon, nullptr, nullptr, nullptr);
}

int orbx_lk_track_window_fb(orbx_ctx* c, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                            size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen,
                            float* err, int win_size, int max_level, int max_iters, double epsilon, float fb_threshold,
                            float* fb_d2, int32_t* lost) {
  return lkw_window_host(c, frames, n_frames, width, height, row_stride, frame_stride, pts_xy, n, tracks_xy, seen, err,
                         win_size, max_level, max_iters, epsilon, &fb_threshold, fb_d2, lost);
}

}  // extern "C"
