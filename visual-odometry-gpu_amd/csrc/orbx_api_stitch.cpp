// orbx_api_stitch.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_stream.h: a stream of overlapping
// tracked windows chained, solved and gated window by window in the batched calls, then joined into one trajectory
// (DESIGN.md §9 rank 16).
// cur_pose = prev_pose * T.inv() across solves (src/with_bundle_adjustment.cpp:203), cur_pose = pose_window.back() and
// est_path rewritten from pose_window after each solve (:234-249), for many windows per call.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbx_lm.h"
#include "../../include/orbx_stream.h"
#include "../../include/orbx_vo.h"
#include "orbx_host.h"
#include "orbx_st_math.h"

using namespace orbx_host;

static_assert((int)ORBX_ST_OK == (int)ST_OK && (int)ORBX_ST_BROKEN == (int)ST_BROKEN &&
                  (int)ORBX_ST_SCALE_UNALIGNED == (int)ST_SCALE_UNALIGNED,
              "orbx_st_status");
static_assert(ST_LINK_DOUBLES == 14, "StInput: 14 doubles per link");

namespace {

// the argument rules of a stitch, device or host (c may be NULL: the host entry has no context)
int st_check(orbx_ctx* c, const void* poses, int n, int len, int stride, const double* T_start, int align_scale) {
  if (!poses) return fail(c, ORBX_ERR_INVALID_ARG, "poses4x4 is NULL");
  if (n < 1 || len < 2) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1 or window_len < 2");
  if (stride < 1 || stride > len - 1) return fail(c, ORBX_ERR_INVALID_ARG, "stride outside [1, window_len - 1]");
  if (align_scale && stride == len - 1)
    return fail(c, ORBX_ERR_INVALID_ARG, "align_scale needs two shared frames: stride <= window_len - 2");
  if (T_start && !finite_all(T_start, 16)) return fail(c, ORBX_ERR_INVALID_ARG, "T_start is not finite");
  if (st_frames(n, len, stride) < 1 || (unsigned long long)n * len > 0x7fffffffull / 16)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more stream frames or window poses than 2^27 - 1");
  return ORBX_OK;
}

// enqueues the three kernels of a stitch on s; arguments are checked
int st_run(orbx_ctx* c, const double* d_poses, int n, int len, int stride, const double* T_start, int align_scale,
           hipStream_t s) {
  int st = c->st.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->st.side, s};
  // the poses may be the window-poses block or the write-back block, written on another stream
  if ((st = c->st.side.after(c, c->wp.side, s)) != ORBX_OK) return st;
  const StInput I((size_t)n);
  const StBlock B((size_t)n, (size_t)len, (size_t)stride);
  if ((st = c->st.side.grow(c, c->st.in, I.bytes)) != ORBX_OK) return st;
  if ((st = c->st.side.grow(c, c->st.blk, B.bytes)) != ORBX_OK) return st;
  // from here on the previous block is being replaced (a larger one has already taken its place)
  c->st.n = 0;
  double T[16];
  for (int i = 0; i < 16; i++) T[i] = T_start ? T_start[i] : (i % 5 == 0 ? 1.0 : 0.0);
  if ((st = c->st.up.send(c, at<double>(c->st.in, I.T_start), T, sizeof T, s)) != ORBX_OK) return st;
  HIPCHK(c, orbx_launch_stitch(s, n, len, stride, d_poses, at<const double>(c->st.in, I.T_start), align_scale,
                               at<double>(c->st.in, I.links), at<int32_t>(c->st.in, I.broken),
                               at<double>(c->st.blk, B.trajectory4x4), at<int32_t>(c->st.blk, B.owner),
                               at<double>(c->st.blk, B.anchors4x4), at<double>(c->st.blk, B.lambda),
                               at<int32_t>(c->st.blk, B.status)));
  c->st.n = n;
  c->st.len = len;
  c->st.stride = stride;
  return ORBX_OK;
}

StBlock st_block(const orbx_ctx* c) { return StBlock((size_t)c->st.n, (size_t)c->st.len, (size_t)c->st.stride); }

// whether the stream's landmarks come from the build of rank 10 on the chained poses (the reference's) or from the
// views build of rank 15
bool st_plain_build(int tri_mode, double max_reproj_px) { return tri_mode == ORBX_LM_TRI_FIRST_TWO && max_reproj_px == 0.0; }

// every stage's argument rules, before the first launch
int st_check_stream(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len,
                    int stride, const double* T_start, double scale0_first, double prob, double threshold,
                    int pose_max_iters, int tri_mode, double max_reproj_px, double huber_delta, int ba_max_iters,
                    double max_rot, double max_trans, int align_scale) {
  int st = lm_check_build(c, K, tracks, seen, n, cap, len, nullptr);
  if (st != ORBX_OK) return st;
  if ((st = tp_check(c, K, tracks, seen, n, cap, len, prob, threshold, pose_max_iters)) != ORBX_OK) return st;
  if (!std::isfinite(scale0_first)) return fail(c, ORBX_ERR_INVALID_ARG, "scale0_first is not finite");
  if (!lm_views_ok(LmViewsOptions{tri_mode, max_reproj_px}))
    return fail(c, ORBX_ERR_INVALID_ARG, "tri_mode outside 0..2, or max_reproj_px negative or not finite");
  if (!ba_params_ok(huber_delta, ba_max_iters) || !gate_params_ok(max_rot, max_trans))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment or write-back arguments");
  return st_check(c, tracks, n, len, stride, T_start, align_scale);
}

// the six stages on s; arguments are checked
int st_run_stream(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
                  int stride, const double* T_start, double scale0_first, double prob, double threshold,
                  int pose_max_iters, uint64_t seed, int tri_mode, double max_reproj_px, double huber_delta,
                  int ba_max_iters, double max_rot, double max_trans, int align_scale, hipStream_t s) {
  int st = orbx_tracks_pose_device(c, K, d_tracks, d_seen, n, cap, len, prob, threshold, pose_max_iters, seed, s);
  if (st != ORBX_OK) return st;
  const WpStreamOptions o{stride, scale0_first};
  if ((st = wp_run(c, nullptr, nullptr, s, &o)) != ORBX_OK) return st;
  st = st_plain_build(tri_mode, max_reproj_px)
           ? orbx_landmarks_build_chained_device(c, K, d_tracks, d_seen, n, cap, len, s)
           : orbx_landmarks_build_views_device(c, K, d_tracks, d_seen, n, cap, len, nullptr, tri_mode, max_reproj_px, s);
  if (st != ORBX_OK) return st;
  if ((st = orbx_bundle_adjust_landmarks_device(c, huber_delta, ba_max_iters, s)) != ORBX_OK) return st;
  if ((st = orbx_bundle_adjust_write_back_device(c, max_rot, max_trans, s)) != ORBX_OK) return st;
  const WbBlock B((size_t)c->wp.wb_n, (size_t)c->wp.wb_len);
  return st_run(c, at<const double>(c->wp.wb, B.poses4x4), n, len, stride, T_start, align_scale, s);
}

}  // namespace

extern "C" {

int orbx_window_poses_stream_device(orbx_ctx* c, int stride, double scale0_first, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const WpStreamOptions o{stride, scale0_first};
  return wp_run(c, nullptr, nullptr, stream_of(c, stream), &o);
}

int orbx_stitch_windows_device(orbx_ctx* c, const double* d_poses4x4, int n_windows, int window_len, int stride,
                               const double* T_start, int align_scale, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = st_check(c, d_poses4x4, n_windows, window_len, stride, T_start, align_scale);
  if (st != ORBX_OK) return st;
  return st_run(c, d_poses4x4, n_windows, window_len, stride, T_start, align_scale, stream_of(c, stream));
}

int orbx_stitch_results_device(orbx_ctx* c, orbx_stitch_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->st.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no windows have been stitched");
  const StBlock B = st_block(c);
  v->trajectory4x4 = at<const double>(c->st.blk, B.trajectory4x4);
  v->owner = at<const int32_t>(c->st.blk, B.owner);
  v->anchors4x4 = at<const double>(c->st.blk, B.anchors4x4);
  v->lambda = at<const double>(c->st.blk, B.lambda);
  v->status = at<const int32_t>(c->st.blk, B.status);
  v->n_frames = (int32_t)B.frames;
  v->n_windows = c->st.n;
  v->window_len = c->st.len;
  v->stride = c->st.stride;
  return ORBX_OK;
}

int orbx_stitch_fetch(orbx_ctx* c, int first_frame, int n_frames, double* trajectory4x4, int32_t* owner,
                      int first_window, int n_windows, double* anchors4x4, double* lambda, int32_t* status) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->st.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no windows have been stitched");
  const StBlock B = st_block(c);
  const bool frames = trajectory4x4 || owner, windows = anchors4x4 || lambda || status;
  if (frames && !range_ok(first_frame, n_frames, (int)B.frames))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first_frame, first_frame + n_frames) outside the stream");
  if (windows && !range_ok(first_window, n_windows, c->st.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first_window, first_window + n_windows) outside the stitch block");
  const int st = c->st.side.wait(c);
  if (st != ORBX_OK) return st;
  const size_t f0 = (size_t)first_frame, nf = (size_t)n_frames, w0 = (size_t)first_window, nw = (size_t)n_windows;
  if (trajectory4x4)
    HIPCHK(c, hipMemcpy(trajectory4x4, at<const double>(c->st.blk, B.trajectory4x4) + 16 * f0, sizeof(double) * 16 * nf,
                        hipMemcpyDeviceToHost));
  if (owner)
    HIPCHK(c, hipMemcpy(owner, at<const int32_t>(c->st.blk, B.owner) + f0, sizeof(int32_t) * nf, hipMemcpyDeviceToHost));
  if (anchors4x4)
    HIPCHK(c, hipMemcpy(anchors4x4, at<const double>(c->st.blk, B.anchors4x4) + 16 * w0, sizeof(double) * 16 * nw,
                        hipMemcpyDeviceToHost));
  if (lambda)
    HIPCHK(c, hipMemcpy(lambda, at<const double>(c->st.blk, B.lambda) + w0, sizeof(double) * nw, hipMemcpyDeviceToHost));
  if (status)
    HIPCHK(c, hipMemcpy(status, at<const int32_t>(c->st.blk, B.status) + w0, sizeof(int32_t) * nw, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_stitch_windows(const double* poses4x4, int n_windows, int window_len, int stride, const double* T_start,
                        int align_scale, double* trajectory4x4, int32_t* owner, double* anchors4x4, double* lambda,
                        int32_t* status) {
  const int chk = st_check(nullptr, poses4x4, n_windows, window_len, stride, T_start, align_scale);
  if (chk != ORBX_OK) return chk;
  const size_t W = (size_t)n_windows, F = (size_t)st_frames(n_windows, window_len, stride);
  std::vector<double> links(ST_LINK_DOUBLES * W), anchors(16 * W), lam(W);
  std::vector<int32_t> broken(W), stat(W);
  for (size_t w = 0; w < W; w++)
    broken[w] = st_link(poses4x4 + 16 * w * window_len, window_len, stride, &links[ST_LINK_DOUBLES * w]);
  double G[16], Lam;
  st_fold_begin(T_start, G, &Lam);
  for (size_t w = 0; w < W; w++)
    stat[w] = st_fold_step((int)w, &links[ST_LINK_DOUBLES * w], broken[w],
                           w ? links[ST_LINK_DOUBLES * (w - 1) + 13] : 0.0, align_scale, G, &Lam, &anchors[16 * w],
                           &lam[w]);
  for (size_t f = 0; f < F; f++) {
    double T[16];
    const int o = st_apply((int)f, n_windows, window_len, stride, poses4x4, anchors.data(), lam.data(), stat.data(), T);
    if (trajectory4x4) std::memcpy(trajectory4x4 + 16 * f, T, sizeof T);
    if (owner) owner[f] = o;
  }
  if (anchors4x4) std::memcpy(anchors4x4, anchors.data(), sizeof(double) * anchors.size());
  if (lambda) std::memcpy(lambda, lam.data(), sizeof(double) * W);
  if (status) std::memcpy(status, stat.data(), sizeof(int32_t) * W);
  return ORBX_OK;
}

int orbx_stream_odometry_tracks_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                       int n_windows, int slot_capacity, int window_len, int stride,
                                       const double* T_start, double scale0_first, double prob, double threshold,
                                       int pose_max_iters, uint64_t seed, int tri_mode, double max_reproj_px,
                                       double huber_delta, int ba_max_iters, double max_rot, double max_trans,
                                       int align_scale, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = st_check_stream(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, stride, T_start,
                                 scale0_first, prob, threshold, pose_max_iters, tri_mode, max_reproj_px, huber_delta,
                                 ba_max_iters, max_rot, max_trans, align_scale);
  if (st != ORBX_OK) return st;
  return st_run_stream(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, stride, T_start, scale0_first,
                       prob, threshold, pose_max_iters, seed, tri_mode, max_reproj_px, huber_delta, ba_max_iters,
                       max_rot, max_trans, align_scale, stream_of(c, stream));
}

int orbx_stream_odometry_tracks(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen,
                                int n_windows, int n_slots, int window_len, int stride, const double* T_start,
                                double scale0_first, double prob, double threshold, int pose_max_iters, uint64_t seed,
                                int tri_mode, double max_reproj_px, double huber_delta, int ba_max_iters,
                                double max_rot, double max_trans, int align_scale, double* trajectory4x4,
                                int32_t* st_status, int32_t* wp_status, int32_t* lm_status,
                                orbx_ba_summary* summaries) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!trajectory4x4) return fail(c, ORBX_ERR_INVALID_ARG, "trajectory4x4 is NULL");
  int st = st_check_stream(c, K, tracks_xy, seen, n_windows, n_slots, window_len, stride, T_start, scale0_first, prob,
                           threshold, pose_max_iters, tri_mode, max_reproj_px, huber_delta, ba_max_iters, max_rot,
                           max_trans, align_scale);
  if (st != ORBX_OK) return st;
  // [n_windows][n_slots] windows are n_windows * n_slots tracks of one long window to the staging helper
  const float* d_tracks;
  const int32_t* d_seen;
  if ((st = stage_tracks(c, c->st.side, c->st.stage, tracks_xy, seen, n_windows * n_slots, window_len, &d_tracks,
                         &d_seen)) != ORBX_OK)
    return st;
  if ((st = st_run_stream(c, K, d_tracks, d_seen, n_windows, n_slots, window_len, stride, T_start, scale0_first, prob,
                          threshold, pose_max_iters, seed, tri_mode, max_reproj_px, huber_delta, ba_max_iters, max_rot,
                          max_trans, align_scale, c->stream)) != ORBX_OK)
    return st;
  if ((st = orbx_stitch_fetch(c, 0, st_frames(n_windows, window_len, stride), trajectory4x4, nullptr, 0, n_windows,
                              nullptr, nullptr, st_status)) != ORBX_OK)
    return st;
  if (wp_status && (st = orbx_window_poses_fetch(c, 0, n_windows, nullptr, nullptr, wp_status)) != ORBX_OK) return st;
  if (lm_status && (st = orbx_landmarks_fetch(c, 0, n_windows, lm_status, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              nullptr, nullptr, nullptr, 0, nullptr, nullptr)) != ORBX_OK)
    return st;
  if (summaries) return orbx_bundle_adjust_landmarks_fetch(c, 0, n_windows, nullptr, summaries, nullptr, 0, nullptr);
  return ORBX_OK;
}

}  // extern "C"
