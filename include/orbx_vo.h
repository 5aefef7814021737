/* orbx_vo.h -- the second public header of liborbx.so: the links of the reference's bundle-adjustment loop that close
 * the device chain from tracked windows to gated camera -> world poses.
 *
 *   orbx_lk_track_windows[_fb]_device -> orbx_tracks_pose_device -> orbx_window_poses_device ->
 *   orbx_landmarks_build_chained_device -> orbx_bundle_adjust_landmarks_device ->
 *   orbx_bundle_adjust_write_back_device -> orbx_bundle_adjust_write_back_fetch
 *
 * Two pieces of the reference are replaced:
 *   pair motions -> window poses   T = [R | scale t], cur_pose = prev_pose * T.inv(), pushed into pose_window
 *                                  (src/with_bundle_adjustment.cpp:196-208), and pose_window[i].inv() -> cv::Rodrigues
 *                                  -> the 6-double block of the solve (src/with_bundle_adjustment.cpp:615-628)
 *   solved blocks -> pose_window   only on convergence, and a pose only if it moved by less than MAX_ROT_DIFF and
 *                                  MAX_TRANS_DIFF (src/with_bundle_adjustment.cpp:683-718)
 * Rules (csrc/orbx_wp_math.h holds the arithmetic, tests/cpp/wp_sequential.cpp restates the
 * kernels sequentially and results are bit-identical to it):
 *   chain    per window, C_0 = T0 and C_{k+1} = C_k [R^T | -s R^T t] with pair k's R, t: the product
 *            orbx_chain_trajectory forms, in its operation order; s = scale0 for pair 0, the pair's scale from pair 1 on
 *   blocks   (R_wc, t_wc) = C_k^-1 in closed form, poses6 = (angle-axis of R_wc through the unit quaternion, t_wc)
 *   status   ORBX_WP_NONFINITE when any of the window's numbers is not finite, else ORBX_WP_OK
 *   gate     R_d = R(new) R(old)^T with the rotation matrices of the solve's own pose arithmetic, angle = |log R_d|,
 *            d = |t_new - t_old| on the world -> camera translations; updated = the window's termination is
 *            ORBX_BA_CONVERGENCE and angle < max_rot and d < max_trans; the 4x4 handed out is the inverse of the new
 *            block when updated, of the old block otherwise
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the block it reads when that was written on another stream.  The block an entry reads
 * must not be replaced from another stream while the entry's work is in flight.  On any error nothing is launched or
 * written, the previous results stay fetchable and the context usable. */
#ifndef ORBX_VO_H
#define ORBX_VO_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_WP_OK = 0,
  ORBX_WP_NONFINITE = 1 /* a pair motion, T0 times it, or a block of the window is not finite */
} orbx_wp_status;

/* Chains the LAST tracks-pose block (orbx_tracks_pose_device) into window poses
 * (src/with_bundle_adjustment.cpp:196-208, :615-628): n_windows and window_len are that block's.  T0: host, n_windows
 * row-major 4x4 camera -> world poses of the windows' first frames, NULL: identity.  scale0: host, the scale of every
 * window's pair 0, NULL: 1.0 (the tracks pose has no earlier pair to join pair 0 with).  Both are copied before the
 * call returns.  ORBX_ERR_INVALID_ARG without a tracks-pose block, for a T0 or scale0 that is not finite, and for a
 * window_len above ORBX_BA_MAX_POSES.  The results go to a block of their own. */
int orbx_window_poses_device(orbx_ctx* ctx, const double* T0, const double* scale0, void* stream);
/* Device-side view of the last chain's results (src/with_bundle_adjustment.cpp:196-208, :615-628), valid until the
 * next chain; written on that call's stream. */
typedef struct {
  const double* poses6;   /* [n_windows][window_len][6]: angle-axis, translation, world -> camera */
  const double* poses4x4; /* [n_windows][window_len][16]: camera -> world, row-major */
  const int32_t* status;  /* [n_windows]: orbx_wp_status */
  int32_t window_len;
  int32_t n_windows;
} orbx_window_poses_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before any chain.  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_results_device(orbx_ctx* ctx, orbx_window_poses_view* view);
/* Waits for the last chain and copies windows [first, first + n) in the view's layout; each array may be NULL.
 * src/with_bundle_adjustment.cpp:196-208, :615-628 */
int orbx_window_poses_fetch(orbx_ctx* ctx, int first, int n, double* poses6, double* poses4x4, int32_t* status);
/* One window on the host, no context: the same arithmetic from the same source
 * (src/with_bundle_adjustment.cpp:196-208, :615-628).  T0: 16 doubles, NULL: identity; R, t, scale: n_pairs motions,
 * every scale used as given; poses4x4: (n_pairs + 1) x 16 and poses6: (n_pairs + 1) x 6 out, each may be NULL.  The
 * 4x4 poses are those of orbx_chain_trajectory bit for bit. */
int orbx_chain_window_poses(const double* T0, const double* R, const double* t, const double* scale, int n_pairs,
                            double* poses4x4, double* poses6);
/* orbx_landmarks_build_device with the poses taken from the last window-poses block instead of the host
 * (src/with_bundle_adjustment.cpp:502-575 on the poses of :615-628): n_windows and window_len have to be that
 * block's, else ORBX_ERR_INVALID_ARG; every other rule is orbx_landmarks_build_device's.  A window whose chain is
 * ORBX_WP_NONFINITE becomes ORBX_LM_BAD_POSE and owns no landmark.  The result is the landmarks block: orbx_landmarks_*
 * and orbx_bundle_adjust_landmarks_* work on it unchanged. */
int orbx_landmarks_build_chained_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy,
                                        const int32_t* d_seen, int n_windows, int slot_capacity, int window_len,
                                        void* stream);
/* The write-back gate (src/with_bundle_adjustment.cpp:683-718) on the last SOLVED landmarks block, however it was
 * built: the blocks after orbx_bundle_adjust_landmarks_device against the blocks as built.  The reference's
 * MAX_ROT_DIFF and MAX_TRANS_DIFF are 0.5 and 50.  ORBX_ERR_INVALID_ARG when the block has not been solved and for a
 * max_rot or max_trans that is <= 0 or not finite.  The results go to a block of their own. */
int orbx_bundle_adjust_write_back_device(orbx_ctx* ctx, double max_rot, double max_trans, void* stream);
/* Device-side view of the last write-back's results (src/with_bundle_adjustment.cpp:708-718), valid until the next
 * write-back; written on that call's stream. */
typedef struct {
  const double* poses4x4; /* [n_windows][window_len][16]: camera -> world, row-major: the gated pose_window */
  const uint8_t* updated; /* [n_windows][window_len]: 1 where the solved pose was written back */
  int32_t window_len;
  int32_t n_windows;
} orbx_ba_write_back_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before any write-back.  src/with_bundle_adjustment.cpp:708-718 */
int orbx_bundle_adjust_write_back_results_device(orbx_ctx* ctx, orbx_ba_write_back_view* view);
/* Waits for the last write-back and copies windows [first, first + n) in the view's layout; each array may be NULL.
 * src/with_bundle_adjustment.cpp:683-718 */
int orbx_bundle_adjust_write_back_fetch(orbx_ctx* ctx, int first, int n, double* poses4x4, uint8_t* updated);
/* Host convenience, the twin of orbx_bundle_adjust_tracks: ONE window of host tracks (n_slots x window_len x 2) and
 * seen (n_slots) through tracks pose, chain, landmarks build, solve and write-back as a batch of one
 * (src/with_bundle_adjustment.cpp:180-208, :502-575, :612-720).  T0: 16 doubles or NULL; scale0: the scale of pair 0;
 * prob, threshold, pose_max_iters, seed: orbx_tracks_pose's; huber_delta, ba_max_iters:
 * orbx_bundle_adjust_landmarks_device's; max_rot, max_trans: the gate's.  Out: poses4x4 (window_len x 16) and updated
 * (window_len), required; wp_status, lm_status and summary may be NULL.  Synchronous; replaces the results of all five
 * stages. */
int orbx_window_odometry_tracks(orbx_ctx* ctx, const double* K, const float* tracks_xy, const int32_t* seen,
                                int n_slots, int window_len, const double* T0, double scale0, double prob,
                                double threshold, int pose_max_iters, uint64_t seed, double huber_delta,
                                int ba_max_iters, double max_rot, double max_trans, double* poses4x4,
                                uint8_t* updated, int32_t* wp_status, int32_t* lm_status, orbx_ba_summary* summary);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_VO_H */
