// orbx_api_wposes.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_vo.h: the poses of tracked windows
// chained on the device from the tracks-pose block, the landmarks build that reads them there, and the write-back
// gate behind the solve.
// cur_pose = prev_pose * T.inv() into pose_window (src/with_bundle_adjustment.cpp:196-208), pose_window[i].inv() ->
// cv::Rodrigues -> the 6-double block (:615-628) and the gate of :683-718, for many windows per call.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbx_vo.h"
#include "orbx_host.h"
#include "orbx_wp_math.h"

using namespace orbx_host;

static_assert((int)ORBX_WP_OK == (int)WP_OK && (int)ORBX_WP_NONFINITE == (int)WP_NONFINITE, "orbx_wp_status");

namespace {

int wp_check_range(orbx_ctx* c, int first, int n, int total, const char* none, const char* outside) {
  if (total < 1) return fail(c, ORBX_ERR_INVALID_ARG, none);
  if (!range_ok(first, n, total)) return fail(c, ORBX_ERR_INVALID_ARG, outside);
  return ORBX_OK;
}

}  // namespace

namespace orbx_host {

bool gate_params_ok(double max_rot, double max_trans) {
  return max_rot > 0.0 && std::isfinite(max_rot) && max_trans > 0.0 && std::isfinite(max_trans);
}

// the argument rules of a chain of the last tracks-pose block; nothing is launched
int wp_check(orbx_ctx* c, const double* T0, const double* scale0, const WpStreamOptions* stream_of_windows) {
  const int n = c->tp.n, len = c->tp.len;
  if (n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no tracks have been posed");
  if (len > ORBX_BA_MAX_POSES) return fail(c, ORBX_ERR_INVALID_ARG, "window_len above ORBX_BA_MAX_POSES");
  if ((T0 && !finite_all(T0, 16 * n)) || (scale0 && !finite_all(scale0, n)))
    return fail(c, ORBX_ERR_INVALID_ARG, "T0 or scale0 is not finite");
  if (stream_of_windows) {
    if (stream_of_windows->stride < 1 || stream_of_windows->stride > len - 1)
      return fail(c, ORBX_ERR_INVALID_ARG, "stride outside [1, window_len - 1]");
    if (!std::isfinite(stream_of_windows->scale0_first))
      return fail(c, ORBX_ERR_INVALID_ARG, "scale0_first is not finite");
  }
  return ORBX_OK;
}

// the chain of the last tracks-pose block on s; T0 / scale0: host or NULL
int wp_run(orbx_ctx* c, const double* T0, const double* scale0, hipStream_t s,
           const WpStreamOptions* stream_of_windows) {
  int st = wp_check(c, T0, scale0, stream_of_windows);
  if (st != ORBX_OK) return st;
  const int n = c->tp.n, len = c->tp.len;
  if ((st = c->wp.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->wp.side, s};
  // the tracks-pose block may have been written on another stream
  if ((st = c->wp.side.after(c, c->tp.side, s)) != ORBX_OK) return st;
  const WpInput I((size_t)n);
  const WpBlock B((size_t)n, (size_t)len);
  if ((st = c->wp.side.grow(c, c->wp.in, I.bytes)) != ORBX_OK) return st;
  if ((st = c->wp.side.grow(c, c->wp.blk, B.bytes)) != ORBX_OK) return st;
  // from here on the previous block is being replaced (a larger one has already taken its place)
  c->wp.n = 0;
  std::vector<uint8_t> up(I.bytes, 0);
  double* hT0 = reinterpret_cast<double*>(up.data() + I.T0);
  double* hs0 = reinterpret_cast<double*>(up.data() + I.scale0);
  for (int w = 0; w < n; w++) {
    for (int i = 0; i < 16; i++) hT0[16 * (size_t)w + i] = T0 ? T0[16 * (size_t)w + i] : (i % 5 == 0 ? 1.0 : 0.0);
    hs0[w] = scale0 ? scale0[w] : 1.0;
  }
  if ((st = c->wp.up.send(c, c->wp.in.p, up.data(), I.bytes, s)) != ORBX_OK) return st;
  const TpBlock P((size_t)n, (size_t)c->tp.cap, (size_t)len);
  // a stream of overlapping windows: pair 0's scale of window w + 1 is window w's, gathered behind the upload
  if (stream_of_windows)
    HIPCHK(c, orbx_launch_st_scale0(s, n, len, stream_of_windows->stride, stream_of_windows->scale0_first,
                                    at<const OrbxScaleOut>(c->tp.blk, P.scale), at<double>(c->wp.in, I.scale0)));
  HIPCHK(c, orbx_launch_window_poses(s, n, len, at<const OrbxPoseOut>(c->tp.blk, P.pose),
                                     at<const OrbxScaleOut>(c->tp.blk, P.scale), at<const double>(c->wp.in, I.T0),
                                     at<const double>(c->wp.in, I.scale0), at<double>(c->wp.blk, B.poses6),
                                     at<double>(c->wp.blk, B.poses4x4), at<int32_t>(c->wp.blk, B.status)));
  c->wp.n = n;
  c->wp.len = len;
  return ORBX_OK;
}

}  // namespace orbx_host

extern "C" {

int orbx_window_poses_device(orbx_ctx* c, const double* T0, const double* scale0, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return wp_run(c, T0, scale0, stream_of(c, stream));
}

int orbx_window_poses_results_device(orbx_ctx* c, orbx_window_poses_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->wp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no window poses have been chained");
  const WpBlock B((size_t)c->wp.n, (size_t)c->wp.len);
  v->poses6 = at<const double>(c->wp.blk, B.poses6);
  v->poses4x4 = at<const double>(c->wp.blk, B.poses4x4);
  v->status = at<const int32_t>(c->wp.blk, B.status);
  v->window_len = c->wp.len;
  v->n_windows = c->wp.n;
  return ORBX_OK;
}

int orbx_window_poses_fetch(orbx_ctx* c, int first, int n, double* poses6, double* poses4x4, int32_t* status) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = wp_check_range(c, first, n, c->wp.n, "no window poses have been chained",
                          "[first, first + n) outside the window-poses block");
  if (st != ORBX_OK) return st;
  if ((st = c->wp.side.wait(c)) != ORBX_OK) return st;
  const WpBlock B((size_t)c->wp.n, (size_t)c->wp.len);
  const size_t frames = (size_t)n * c->wp.len, f0 = (size_t)first * c->wp.len;
  if (poses6)
    HIPCHK(c, hipMemcpy(poses6, at<const double>(c->wp.blk, B.poses6) + 6 * f0, sizeof(double) * 6 * frames,
                        hipMemcpyDeviceToHost));
  if (poses4x4)
    HIPCHK(c, hipMemcpy(poses4x4, at<const double>(c->wp.blk, B.poses4x4) + 16 * f0, sizeof(double) * 16 * frames,
                        hipMemcpyDeviceToHost));
  if (status)
    HIPCHK(c, hipMemcpy(status, at<const int32_t>(c->wp.blk, B.status) + first, sizeof(int32_t) * (size_t)n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_chain_window_poses(const double* T0, const double* R, const double* t, const double* scale, int n_pairs,
                            double* poses4x4, double* poses6) {
  if (n_pairs < 0 || (n_pairs > 0 && (!R || !t || !scale))) return ORBX_ERR_INVALID_ARG;
  const size_t L = (size_t)n_pairs + 1;
  std::vector<double> p4(16 * L), p6(6 * L);
  // pair 0's scale is the chain's scale0; from pair 1 on wp_chain_window reads scale[k]
  (void)wp_chain_window(T0, R, 9, t, 3, scale, 1, n_pairs > 0 ? scale[0] : 1.0, (int)L, p4.data(), p6.data());
  if (poses4x4) std::memcpy(poses4x4, p4.data(), sizeof(double) * p4.size());
  if (poses6) std::memcpy(poses6, p6.data(), sizeof(double) * p6.size());
  return ORBX_OK;
}

int orbx_landmarks_build_chained_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                        int n_windows, int slot_capacity, int window_len, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = lm_check_build(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, nullptr);
  if (st != ORBX_OK) return st;
  if (c->wp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no window poses have been chained");
  if (n_windows != c->wp.n || window_len != c->wp.len)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows or window_len differs from the window-poses block");
  const WpBlock B((size_t)c->wp.n, (size_t)c->wp.len);
  return lm_run(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, nullptr,
                at<const double>(c->wp.blk, B.poses6), at<const int32_t>(c->wp.blk, B.status), stream_of(c, stream));
}

int orbx_bundle_adjust_write_back_device(orbx_ctx* c, double max_rot, double max_trans, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!gate_params_ok(max_rot, max_trans))
    return fail(c, ORBX_ERR_INVALID_ARG, "max_rot or max_trans is not > 0 and finite");
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (!c->lm.solved) return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has not been solved");
  hipStream_t s = stream_of(c, stream);
  int st = c->wp.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->wp.side, s};
  // the solve may have run on another stream
  if ((st = c->wp.side.after(c, c->lm.side, s)) != ORBX_OK) return st;
  const int n = c->lm.n, len = c->lm.len;
  const WbBlock B((size_t)n, (size_t)len);
  if ((st = c->wp.side.grow(c, c->wp.wb, B.bytes)) != ORBX_OK) return st;
  c->wp.wb_n = 0;
  const LmScratch S((size_t)n, c->lm.cap, (size_t)len);
  const LmSolve V((size_t)n, (size_t)c->lm.cap, (size_t)len);
  HIPCHK(c, orbx_launch_ba_write_back(s, n, len, at<const double>(c->lm.sol, V.poses),
                                      at<const double>(c->lm.scr, S.poses), at<const uint8_t>(c->lm.sol, V.out), max_rot,
                                      max_trans, at<double>(c->wp.wb, B.poses4x4), at<uint8_t>(c->wp.wb, B.updated)));
  c->wp.wb_n = n;
  c->wp.wb_len = len;
  return ORBX_OK;
}

int orbx_bundle_adjust_write_back_results_device(orbx_ctx* c, orbx_ba_write_back_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->wp.wb_n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no write-back has run");
  const WbBlock B((size_t)c->wp.wb_n, (size_t)c->wp.wb_len);
  v->poses4x4 = at<const double>(c->wp.wb, B.poses4x4);
  v->updated = at<const uint8_t>(c->wp.wb, B.updated);
  v->window_len = c->wp.wb_len;
  v->n_windows = c->wp.wb_n;
  return ORBX_OK;
}

int orbx_bundle_adjust_write_back_fetch(orbx_ctx* c, int first, int n, double* poses4x4, uint8_t* updated) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = wp_check_range(c, first, n, c->wp.wb_n, "no write-back has run",
                          "[first, first + n) outside the write-back block");
  if (st != ORBX_OK) return st;
  if ((st = c->wp.side.wait(c)) != ORBX_OK) return st;
  const WbBlock B((size_t)c->wp.wb_n, (size_t)c->wp.wb_len);
  const size_t frames = (size_t)n * c->wp.wb_len, f0 = (size_t)first * c->wp.wb_len;
  if (poses4x4)
    HIPCHK(c, hipMemcpy(poses4x4, at<const double>(c->wp.wb, B.poses4x4) + 16 * f0, sizeof(double) * 16 * frames,
                        hipMemcpyDeviceToHost));
  if (updated)
    HIPCHK(c, hipMemcpy(updated, at<const uint8_t>(c->wp.wb, B.updated) + f0, frames, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_window_odometry_tracks(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots,
                                int window_len, const double* T0, double scale0, double prob, double threshold,
                                int pose_max_iters, uint64_t seed, double huber_delta, int ba_max_iters,
                                double max_rot, double max_trans, double* poses4x4, uint8_t* updated,
                                int32_t* wp_status, int32_t* lm_status, orbx_ba_summary* summary) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  // every stage's argument rules first: a refusal launches nothing
  int st = lm_check_build(c, K, tracks_xy, seen, 1, n_slots, window_len, nullptr);
  if (st != ORBX_OK) return st;
  if (!pose_args_ok(K, prob, threshold, pose_max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if ((size_t)n_slots * 16 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots per window than the join holds in LDS");
  if (!ba_params_ok(huber_delta, ba_max_iters) || !gate_params_ok(max_rot, max_trans) || !poses4x4 || !updated)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment or write-back arguments");
  if ((T0 && !finite_all(T0, 16)) || !std::isfinite(scale0))
    return fail(c, ORBX_ERR_INVALID_ARG, "T0 or scale0 is not finite");
  const float* d_tracks;
  const int32_t* d_seen;
  if ((st = stage_tracks(c, c->wp.side, c->wp.stage, tracks_xy, seen, n_slots, window_len, &d_tracks, &d_seen)) != ORBX_OK)
    return st;
  if ((st = orbx_tracks_pose_device(c, K, d_tracks, d_seen, 1, n_slots, window_len, prob, threshold, pose_max_iters,
                                    seed, nullptr)) != ORBX_OK)
    return st;
  if ((st = wp_run(c, T0, &scale0, c->stream)) != ORBX_OK) return st;
  if ((st = orbx_landmarks_build_chained_device(c, K, d_tracks, d_seen, 1, n_slots, window_len, nullptr)) != ORBX_OK)
    return st;
  if ((st = orbx_bundle_adjust_landmarks_device(c, huber_delta, ba_max_iters, nullptr)) != ORBX_OK) return st;
  if ((st = orbx_bundle_adjust_write_back_device(c, max_rot, max_trans, nullptr)) != ORBX_OK) return st;
  if ((st = orbx_bundle_adjust_write_back_fetch(c, 0, 1, poses4x4, updated)) != ORBX_OK) return st;
  if (wp_status && (st = orbx_window_poses_fetch(c, 0, 1, nullptr, nullptr, wp_status)) != ORBX_OK) return st;
  if (lm_status && (st = orbx_landmarks_fetch(c, 0, 1, lm_status, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              nullptr, nullptr, nullptr, 0, nullptr, nullptr)) != ORBX_OK)
    return st;
  if (summary) return orbx_bundle_adjust_landmarks_fetch(c, 0, 1, nullptr, summary, nullptr, 0, nullptr);
  return ORBX_OK;
}

}  // extern "C"
