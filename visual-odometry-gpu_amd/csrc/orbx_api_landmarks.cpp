// orbx_api_landmarks.cpp -- host layer of liborbx.so (orbx_host.h): landmarks of tracked windows built on the device
// and their bundle adjustment on that block, and the entries of include/orbx_lm.h: the same
// block built from every view of a track, with a reprojection gate and per-slot diagnostics (rank 15).
// buildLandmarksFromFirstTwoFramesAndTracks (src/with_bundle_adjustment.cpp:502-575) and the solve of the window
// (src/with_bundle_adjustment.cpp:612-720) for many windows per call.  The build behind orbx_landmarks_build_device
// (poses from the host) is also the build behind orbx_landmarks_build_chained_device (orbx_api_wposes.cpp: poses from
// the window-poses block on the device, rank 14).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/orbx_lm.h"
#include "orbx_host.h"
#include "orbx_lm_math.h"

using namespace orbx_host;

static_assert((int)ORBX_LM_TRI_FIRST_TWO == (int)LM_TRI_FIRST_TWO && (int)ORBX_LM_TRI_ALL_VIEWS == (int)LM_TRI_ALL_VIEWS,
              "orbx_lm_tri_mode");
static_assert((int)ORBX_LM_KEPT == (int)LM_KEPT && (int)ORBX_LM_NO_WINDOW == (int)LM_NO_WINDOW, "orbx_lm_reason");

namespace {

OrbxLmBlock lm_pointers(const orbx_ctx* c, const LmBlock& L) {
  uint8_t* b = (uint8_t*)c->lm.blk.p;
  OrbxLmBlock o;
  o.status = (int32_t*)(b + L.status);
  o.pose_off = (int32_t*)(b + L.pose_off);
  o.pt_off = (int32_t*)(b + L.pt_off);
  o.obs_off = (int32_t*)(b + L.obs_off);
  o.points3 = (double*)(b + L.points);
  o.rows = (int32_t*)(b + L.rows);
  o.opose = b + L.opose;
  o.oxy = (double*)(b + L.oxy);
  o.slot_of_point = (int32_t*)(b + L.slot);
  return o;
}

int lm_check_range(orbx_ctx* c, int first, int n) {
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (!range_ok(first, n, c->lm.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the landmarks block");
  return ORBX_OK;
}

int lm_check_views(orbx_ctx* c, int first, int n) {
  if (c->lm.n < 1 || !c->lm.has_views)
    return fail(c, ORBX_ERR_INVALID_ARG, "the last landmarks build was not a views build");
  if (!range_ok(first, n, c->lm.n))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the landmarks block");
  return ORBX_OK;
}

// the pose source of a views build: the host's poses6, or the last window-poses block (poses6 == NULL)
int lm_build_views(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
                   const double* poses6, const LmViewsOptions& o, hipStream_t s) {
  const int st = lm_check_build(c, K, d_tracks, d_seen, n, cap, len, poses6);
  if (st != ORBX_OK) return st;
  if (!lm_views_ok(o))
    return fail(c, ORBX_ERR_INVALID_ARG, "tri_mode outside 0..2, or max_reproj_px negative or not finite");
  if (poses6) return lm_run(c, K, d_tracks, d_seen, n, cap, len, poses6, nullptr, nullptr, s, &o);
  if (c->wp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no window poses have been chained");
  if (n != c->wp.n || len != c->wp.len)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows or window_len differs from the window-poses block");
  const WpBlock B((size_t)c->wp.n, (size_t)c->wp.len);
  return lm_run(c, K, d_tracks, d_seen, n, cap, len, nullptr, at<const double>(c->wp.blk, B.poses6),
                at<const int32_t>(c->wp.blk, B.status), s, &o);
}

// one window of host tracks through a build (views: NULL for rank 10's) and the solve
int lm_tracks(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots, int window_len,
              double* poses6, double huber_delta, int max_iters, int32_t* lm_status, orbx_ba_summary* summary,
              double* points3, int32_t* slot_of_point, int capacity, int* count, const LmViewsOptions* views) {
  if (!poses6) return fail(c, ORBX_ERR_INVALID_ARG, "K, tracks, seen or poses6 is NULL");
  int st = lm_check_build(c, K, tracks_xy, seen, 1, n_slots, window_len, poses6);
  if (st != ORBX_OK) return st;
  if (views && !lm_views_ok(*views))
    return fail(c, ORBX_ERR_INVALID_ARG, "tri_mode outside 0..2, or max_reproj_px negative or not finite");
  if (!ba_params_ok(huber_delta, max_iters) || !lm_status || !summary || capacity < 0)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  const float* d_tracks;
  const int32_t* d_seen;
  if ((st = stage_tracks(c, c->lm.side, c->lm.stage, tracks_xy, seen, n_slots, window_len, &d_tracks, &d_seen)) != ORBX_OK)
    return st;
  if ((st = lm_run(c, K, d_tracks, d_seen, 1, n_slots, window_len, poses6, nullptr, nullptr, c->stream, views)) != ORBX_OK)
    return st;
  if ((st = orbx_bundle_adjust_landmarks_device(c, huber_delta, max_iters, nullptr)) != ORBX_OK) return st;
  int np = 0;
  if ((st = orbx_bundle_adjust_landmarks_fetch(c, 0, 1, nullptr, nullptr, nullptr, 0, &np)) != ORBX_OK) return st;
  if (count) *count = np;
  if ((points3 || slot_of_point) && np > capacity)
    return fail(c, ORBX_ERR_CAPACITY, "bundle_adjust_tracks: capacity is too small");
  if ((st = orbx_landmarks_fetch(c, 0, 1, lm_status, nullptr, nullptr, nullptr, nullptr, slot_of_point, capacity,
                                 nullptr, nullptr, nullptr, 0, nullptr, nullptr)) != ORBX_OK)
    return st;
  return orbx_bundle_adjust_landmarks_fetch(c, 0, 1, poses6, summary, points3, capacity, nullptr);
}

}  // namespace

namespace orbx_host {

bool lm_views_ok(const LmViewsOptions& o) {
  return o.tri_mode >= LM_TRI_FIRST_TWO && o.tri_mode <= LM_TRI_ALL_VIEWS && o.max_reproj_px >= 0.0 &&
         std::isfinite(o.max_reproj_px);
}

bool ba_params_ok(double huber_delta, int max_iters) {
  return huber_delta > 0.0 && std::isfinite(huber_delta) && max_iters >= 1 && max_iters <= 1000;
}

// enqueues the kernels of a build on s (views: those of rank 15, with its options); arguments are checked
int lm_run(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
           const double* poses6, const double* d_poses6, const int32_t* d_pose_status, hipStream_t s,
           const LmViewsOptions* views, const SideWork* producer) {
  int st = c->lm.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->lm.side, s};
  // the tracks may be the windows tracker's block, written on another stream; so may the chained poses
  if ((st = c->lm.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  if (!poses6 && (st = c->lm.side.after(c, producer ? *producer : c->wp.side, s)) != ORBX_OK) return st;
  const LmBlock B(n, cap, len);
  const LmScratch S(n, cap, len);
  if ((st = c->lm.side.grow(c, c->lm.scr, S.bytes)) != ORBX_OK) return st;
  const LmViews V(n, cap, len);
  if (views && (st = c->lm.side.grow(c, c->lm.views, V.bytes)) != ORBX_OK) return st;
  if ((st = c->lm.side.grow(c, c->lm.blk, B.bytes)) != ORBX_OK) return st;
  // from here on the previous block is being replaced (a larger one has already taken its place), and with it the
  // diagnostics of a views build
  c->lm.n = 0;
  c->lm.solved = false;
  c->lm.has_views = false;
  uint8_t* scr = (uint8_t*)c->lm.scr.p;
  const size_t pose_bytes = sizeof(double) * 6 * (size_t)n * len;
  if (poses6) {
    if ((st = c->lm.poses_up.send(c, scr + S.poses, poses6, pose_bytes, s)) != ORBX_OK) return st;
  } else {
    // the solve and the write-back gate read the block as built from here, whatever the next chain writes
    HIPCHK(c, hipMemcpyAsync(scr + S.poses, d_poses6, pose_bytes, hipMemcpyDeviceToDevice, s));
  }
  const int32_t* pose_status = poses6 ? nullptr : d_pose_status;
  if (views)
    HIPCHK(c, orbx_launch_landmarks_views(s, K, (const double*)(scr + S.poses), d_tracks, d_seen, n, cap, len,
                                          views->tri_mode, views->max_reproj_px, at<double>(c->lm.views, V.table),
                                          at<uint8_t>(c->lm.views, V.reason), at<float>(c->lm.views, V.reproj_px),
                                          (double*)(scr + S.cand), scr + S.keep, (int32_t*)(scr + S.partial),
                                          (int32_t*)(scr + S.gate), lm_pointers(c, B), pose_status));
  else
    HIPCHK(c, orbx_launch_landmarks(s, K, (const double*)(scr + S.poses), d_tracks, d_seen, n, cap, len,
                                    (double*)(scr + S.cand), scr + S.keep, (int32_t*)(scr + S.partial),
                                    (int32_t*)(scr + S.gate), lm_pointers(c, B), pose_status));
  std::memcpy(c->lm.K, K, sizeof c->lm.K);
  c->lm.has_views = views != nullptr;
  c->lm.gen++;
  c->lm.n = n;
  c->lm.cap = cap;
  c->lm.len = len;
  return ORBX_OK;
}

int lm_check_build(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len,
                   const double* poses6) {
  if (!K || !tracks || !seen) return fail(c, ORBX_ERR_INVALID_ARG, "K, tracks, seen or poses6 is NULL");
  if (n < 1 || cap < 1 || len < 2 || len > ORBX_BA_MAX_POSES)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1, slot_capacity < 1 or window_len outside [2, 8]");
  if (cap > ORBX_BA_MAX_POINTS) return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a window than 65536");
  if ((unsigned long long)n * ((unsigned long long)cap + 1) > 0x7fffffffull ||
      (unsigned long long)n * cap * len > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks or observations in a batch than 32-bit offsets hold");
  if (!finite_all(K, 9)) return fail(c, ORBX_ERR_INVALID_ARG, "K is not finite");
  for (size_t i = 0; poses6 && i < 6 * (size_t)n * len; i++)
    if (!std::isfinite(poses6[i])) return fail(c, ORBX_ERR_INVALID_ARG, "a pose is not finite");
  return ORBX_OK;
}

// the solve behind orbx_bundle_adjust_landmarks_device and orbx_bundle_adjust_landmarks_pnp_device
int lm_solve(orbx_ctx* c, double huber_delta, int max_iters, hipStream_t s, const double* d_poses6,
             const SideWork* producer, const double* d_prior, int start) {
  if (!ba_params_ok(huber_delta, max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  int st = c->lm.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->lm.side, s};
  if (producer && (st = c->lm.side.after(c, *producer, s)) != ORBX_OK) return st;
  const int n = c->lm.n, cap = c->lm.cap, len = c->lm.len, ocap = cap * len;
  const LmWork W(n, cap, len);
  const LmSolve V(n, cap, len);
  if ((st = c->lm.side.grow(c, c->lm.ws, W.bytes)) != ORBX_OK) return st;
  if ((st = c->lm.side.grow(c, c->lm.sol, V.bytes)) != ORBX_OK) return st;
  const OrbxLmBlock P = lm_pointers(c, LmBlock(n, cap, len));
  const LmScratch S(n, cap, len);
  uint8_t* sol = (uint8_t*)c->lm.sol.p;
  uint8_t* ws = (uint8_t*)c->lm.ws.p;
  c->lm.solved = false;
  // the block stays as built: the solve reads and writes copies of its poses and points
  const void* poses_from = d_poses6 ? (const void*)d_poses6 : (const void*)((const uint8_t*)c->lm.scr.p + S.poses);
  HIPCHK(c, hipMemcpyAsync(sol + V.poses, poses_from, sizeof(double) * 6 * (size_t)n * len, hipMemcpyDeviceToDevice,
                           s));
  HIPCHK(c, hipMemcpyAsync(sol + V.points, P.points3, sizeof(double) * 3 * (size_t)n * cap, hipMemcpyDeviceToDevice, s));
  const double K4[4] = {c->lm.K[0], c->lm.K[4], c->lm.K[2], c->lm.K[5]};
  if (d_prior) {
    HIPCHK(c, orbx_launch_ba_prior(s, n, W.groups, max_iters, K4, huber_delta, P.pose_off, P.pt_off, P.obs_off,
                                   (double*)(sol + V.poses), (double*)(sol + V.points), P.rows, P.opose, P.oxy, cap,
                                   ocap, (double*)(ws + W.wp), (double*)(ws + W.wo),
                                   (unsigned long long*)(ws + W.slot), sol + V.out, d_prior, start));
  } else {
    HIPCHK(c, orbx_launch_ba(s, n, W.groups, max_iters, K4, huber_delta, P.pose_off, P.pt_off, P.obs_off,
                             (double*)(sol + V.poses), (double*)(sol + V.points), P.rows, P.opose, P.oxy, cap, ocap,
                             (double*)(ws + W.wp), (double*)(ws + W.wo), (unsigned long long*)(ws + W.slot),
                             sol + V.out));
  }
  c->lm.solved = true;
  return ORBX_OK;
}

}  // namespace orbx_host

extern "C" {

int orbx_landmarks_build_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                int n_windows, int slot_capacity, int window_len, const double* poses6, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!poses6) return fail(c, ORBX_ERR_INVALID_ARG, "K, tracks, seen or poses6 is NULL");
  const int st = lm_check_build(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, poses6);
  if (st != ORBX_OK) return st;
  return lm_run(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, poses6, nullptr, nullptr,
                stream_of(c, stream));
}

int orbx_landmarks_results_device(orbx_ctx* c, orbx_landmarks_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  const OrbxLmBlock P = lm_pointers(c, LmBlock(c->lm.n, c->lm.cap, c->lm.len));
  v->status = P.status;
  v->pose_offset = P.pose_off;
  v->point_offset = P.pt_off;
  v->obs_offset = P.obs_off;
  v->points3 = P.points3;
  v->rows = P.rows;
  v->obs_pose = P.opose;
  v->obs_xy = P.oxy;
  v->slot_of_point = P.slot_of_point;
  v->slot_capacity = c->lm.cap;
  v->window_len = c->lm.len;
  v->n_windows = c->lm.n;
  return ORBX_OK;
}

int orbx_landmarks_fetch(orbx_ctx* c, int first, int n, int32_t* status, int32_t* pose_offset, int32_t* point_offset,
                         int32_t* obs_offset, double* points3, int32_t* slot_of_point, int point_capacity,
                         int32_t* obs_point, int32_t* obs_pose, double* obs_xy, int obs_capacity, int* n_points,
                         int* n_obs) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = lm_check_range(c, first, n);
  if (st != ORBX_OK) return st;
  if (point_capacity < 0 || obs_capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "a capacity is negative");
  if ((st = c->lm.side.wait(c)) != ORBX_OK) return st;
  const OrbxLmBlock P = lm_pointers(c, LmBlock(c->lm.n, c->lm.cap, c->lm.len));
  const size_t noff = (size_t)n + 1;
  std::vector<int32_t> po(noff), oo(noff);
  HIPCHK(c, hipMemcpy(po.data(), P.pt_off + first, sizeof(int32_t) * noff, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(oo.data(), P.obs_off + first, sizeof(int32_t) * noff, hipMemcpyDeviceToHost));
  const int32_t p0 = po[0], o0 = oo[0];
  const size_t np = (size_t)(po[n] - p0), no = (size_t)(oo[n] - o0);
  if (n_points) *n_points = (int)np;
  if (n_obs) *n_obs = (int)no;
  const bool want_pts = points3 || slot_of_point, want_obs = obs_point || obs_pose || obs_xy;
  if ((want_pts && np > (size_t)point_capacity) || (want_obs && no > (size_t)obs_capacity))
    return fail(c, ORBX_ERR_CAPACITY, "landmarks fetch: a capacity is too small");
  std::vector<int32_t> rows;
  std::vector<uint8_t> op;
  if (obs_point && no) {
    rows.resize(np + (size_t)n);  // N + 1 row starts per window
    HIPCHK(c, hipMemcpy(rows.data(), P.rows + p0 + first, sizeof(int32_t) * rows.size(), hipMemcpyDeviceToHost));
  }
  if (obs_pose && no) {
    op.resize(no);
    HIPCHK(c, hipMemcpy(op.data(), P.opose + o0, no, hipMemcpyDeviceToHost));
  }
  if (status) HIPCHK(c, hipMemcpy(status, P.status + first, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (points3 && np) HIPCHK(c, hipMemcpy(points3, P.points3 + 3 * (size_t)p0, sizeof(double) * 3 * np, hipMemcpyDeviceToHost));
  if (slot_of_point && np)
    HIPCHK(c, hipMemcpy(slot_of_point, P.slot_of_point + p0, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
  if (obs_xy && no) HIPCHK(c, hipMemcpy(obs_xy, P.oxy + 2 * (size_t)o0, sizeof(double) * 2 * no, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < noff; i++) {
    if (pose_offset) pose_offset[i] = (int32_t)i * c->lm.len;
    if (point_offset) point_offset[i] = po[i] - p0;
    if (obs_offset) obs_offset[i] = oo[i] - o0;
  }
  for (size_t i = 0; i < op.size(); i++) obs_pose[i] = op[i];
  if (!rows.empty()) {
    for (int w = 0; w < n; w++) {
      const int32_t* row = rows.data() + (po[w] - p0) + w;
      int32_t* dst = obs_point + (oo[w] - o0);
      for (int j = 0; j < po[w + 1] - po[w]; j++)
        for (int o = row[j]; o < row[j + 1]; o++) dst[o] = j;
    }
  }
  return ORBX_OK;
}

int orbx_bundle_adjust_landmarks_device(orbx_ctx* c, double huber_delta, int max_iters, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return lm_solve(c, huber_delta, max_iters, stream_of(c, stream), nullptr, nullptr);
}

int orbx_bundle_adjust_landmarks_fetch(orbx_ctx* c, int first, int n, double* poses6, orbx_ba_summary* summaries,
                                       double* points3, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = lm_check_range(c, first, n);
  if (st != ORBX_OK) return st;
  if (!c->lm.solved) return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has not been solved");
  if (capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "a capacity is negative");
  if ((st = c->lm.side.wait(c)) != ORBX_OK) return st;
  const OrbxLmBlock P = lm_pointers(c, LmBlock(c->lm.n, c->lm.cap, c->lm.len));
  const LmSolve V(c->lm.n, c->lm.cap, c->lm.len);
  const uint8_t* sol = (const uint8_t*)c->lm.sol.p;
  int32_t p0 = 0, p1 = 0;
  HIPCHK(c, hipMemcpy(&p0, P.pt_off + first, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&p1, P.pt_off + first + n, sizeof(int32_t), hipMemcpyDeviceToHost));
  const size_t np = (size_t)(p1 - p0), per_win = sizeof(double) * 6 * (size_t)c->lm.len;
  if (count) *count = (int)np;
  if (points3 && np > (size_t)capacity) return fail(c, ORBX_ERR_CAPACITY, "landmarks solve fetch: capacity is too small");
  if (poses6) HIPCHK(c, hipMemcpy(poses6, sol + V.poses + per_win * first, per_win * n, hipMemcpyDeviceToHost));
  if (summaries)
    HIPCHK(c, hipMemcpy(summaries, sol + V.out + sizeof(orbx_ba_summary) * (size_t)first, sizeof(orbx_ba_summary) * n,
                        hipMemcpyDeviceToHost));
  if (points3 && np)
    HIPCHK(c, hipMemcpy(points3, sol + V.points + sizeof(double) * 3 * (size_t)p0, sizeof(double) * 3 * np,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_bundle_adjust_tracks(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots,
                              int window_len, double* poses6, double huber_delta, int max_iters, int32_t* lm_status,
                              orbx_ba_summary* summary, double* points3, int32_t* slot_of_point, int capacity,
                              int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return lm_tracks(c, K, tracks_xy, seen, n_slots, window_len, poses6, huber_delta, max_iters, lm_status, summary,
                   points3, slot_of_point, capacity, count, nullptr);
}

// ---- include/orbx_lm.h ----

int orbx_landmarks_build_views_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                      int n_windows, int slot_capacity, int window_len, const double* poses6,
                                      int tri_mode, double max_reproj_px, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return lm_build_views(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, poses6,
                        LmViewsOptions{tri_mode, max_reproj_px}, stream_of(c, stream));
}

int orbx_landmarks_views_results_device(orbx_ctx* c, orbx_landmarks_views_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const int st = lm_check_views(c, 0, 1);
  if (st != ORBX_OK) return st;
  const LmViews V(c->lm.n, c->lm.cap, c->lm.len);
  v->reason = at<const uint8_t>(c->lm.views, V.reason);
  v->reproj_px = at<const float>(c->lm.views, V.reproj_px);
  v->slot_capacity = c->lm.cap;
  v->n_windows = c->lm.n;
  return ORBX_OK;
}

int orbx_landmarks_views_fetch(orbx_ctx* c, int first, int n, uint8_t* reason, float* reproj_px) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = lm_check_views(c, first, n);
  if (st != ORBX_OK) return st;
  if ((st = c->lm.side.wait(c)) != ORBX_OK) return st;
  const LmViews V(c->lm.n, c->lm.cap, c->lm.len);
  const size_t s0 = (size_t)first * c->lm.cap, ns = (size_t)n * c->lm.cap;
  if (reason) HIPCHK(c, hipMemcpy(reason, at<const uint8_t>(c->lm.views, V.reason) + s0, ns, hipMemcpyDeviceToHost));
  if (reproj_px)
    HIPCHK(c, hipMemcpy(reproj_px, at<const float>(c->lm.views, V.reproj_px) + s0, sizeof(float) * ns,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_bundle_adjust_tracks_views(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen,
                                    int n_slots, int window_len, double* poses6, double huber_delta, int max_iters,
                                    int32_t* lm_status, orbx_ba_summary* summary, double* points3,
                                    int32_t* slot_of_point, int capacity, int* count, int tri_mode,
                                    double max_reproj_px) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const LmViewsOptions o{tri_mode, max_reproj_px};
  return lm_tracks(c, K, tracks_xy, seen, n_slots, window_len, poses6, huber_delta, max_iters, lm_status, summary,
                   points3, slot_of_point, capacity, count, &o);
}

}  // extern "C"
