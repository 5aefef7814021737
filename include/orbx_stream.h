/* orbx_stream.h -- the fourth public header of liborbx.so: a stream of OVERLAPPING tracked windows joined into one
 * trajectory on the device.
 *
 * The reference walks its frames one by one: cur_pose = prev_pose * T.inv() (src/with_bundle_adjustment.cpp:203), and
 * after every solve cur_pose = pose_window.back() and est_path is rewritten from pose_window
 * (src/with_bundle_adjustment.cpp:234-249), so that the next frames chain from the corrected pose.  Bundle adjustment
 * does not care which rigid frame, or which scale, its window is expressed in, so here every window is chained, built,
 * solved and gated in a frame of its own (first pose = identity) by the batched entries of orbx.h, orbx_vo.h and
 * orbx_lm.h, and only afterwards are the windows put behind one another, by a fold over small rigid products.
 *
 * Stream geometry: n_windows = W windows of window_len = L frames; window w starts at stream frame w * stride,
 * 1 <= stride <= L - 1, so consecutive windows share at least one frame; the stream has F = (W - 1) * stride + L
 * frames.  P(w, k): pose k of window w, camera -> world, row-major 4x4; c(w, k) its camera centre.
 * Rules (csrc/orbx_st_math.h holds the arithmetic, tests/cpp/st_sequential.cpp restates the
 * kernels sequentially and results are bit-identical to it):
 *   owner     stream frame f belongs to window w = min(W - 1, f / stride) at index k = f - w * stride: the latest
 *             window that contains it, as the reference's later solve overwrites the earlier one
 *   motion    rel(w, k) = P(w, 0)^-1 P(w, k), the inverse in closed form, every dot product summed left to right
 *   scale     b_first(w) = |c(w, 1) - c(w, 0)|, b_link(w) = |c(w, stride + 1) - c(w, stride)|.  With align_scale != 0
 *             lambda(w + 1) = b_link(w) / b_first(w + 1); where a baseline or the quotient is 0 or not finite,
 *             lambda = 1 and window w + 1 is ORBX_ST_SCALE_UNALIGNED.  align_scale == 0: every lambda = 1.
 *             Lambda(0) = 1, Lambda(w + 1) = Lambda(w) lambda(w + 1)
 *   broken    a window with an entry that is not finite: every rel(w, .) is the identity, lambda(w) = 1, both its
 *             baselines count as 0, status ORBX_ST_BROKEN: the trajectory stands still across it and stays finite
 *   fold      G(0) = T_start, G(w + 1) = G(w) [R_rel(w, stride) | Lambda(w) t_rel(w, stride)], a LEFT fold in window
 *             order; anchors4x4[w] = G(w), lambda[w] = Lambda(w)
 *   apply     trajectory[f] = G(w) [R_rel(w, k) | Lambda(w) t_rel(w, k)], bottom row exactly 0 0 0 1
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the block it reads when that was written on another stream.  On any error nothing is
 * launched or written, the previous results stay fetchable and the context usable. */
#ifndef ORBX_STREAM_H
#define ORBX_STREAM_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of status[w] */
typedef enum {
  ORBX_ST_OK = 0,
  ORBX_ST_BROKEN = 1,         /* a pose of the window is not finite: it contributes no motion */
  ORBX_ST_SCALE_UNALIGNED = 2 /* align_scale was asked for and a baseline was 0 or not finite: lambda = 1 */
} orbx_st_status;

/* orbx_window_poses_device (include/orbx_vo.h) for a stream: chains the LAST tracks-pose block into the window-poses
 * block, every window from the identity (src/with_bundle_adjustment.cpp:203 per window).  scale0 of window 0 is
 * scale0_first; of window w >= 1 it is the scale the tracks-pose block holds for pair `stride` of window w - 1 (pair
 * index (w - 1) * (L - 1) + stride, the same two frames as pair 0 of window w), gathered on the device; with
 * stride == L - 1 no such pair exists and it is 1.0.  Refusals: those of orbx_window_poses_device, and
 * ORBX_ERR_INVALID_ARG for a stride outside [1, L - 1] and a scale0_first that is not finite. */
int orbx_window_poses_stream_device(orbx_ctx* ctx, int stride, double scale0_first, void* stream);
/* Joins n_windows windows of window_len poses (src/with_bundle_adjustment.cpp:203, :234-249: the chain across solves
 * and est_path rewritten from pose_window).  d_poses4x4: DEVICE, [n_windows][window_len][16]; it may be
 * orbx_ba_write_back_view.poses4x4 or orbx_window_poses_view.poses4x4, and a call on another stream than the one that
 * block was written on waits for it on the device.  T_start: HOST, 16 doubles, the pose of stream frame 0, NULL:
 * identity; copied before the call returns.  ORBX_ERR_INVALID_ARG for a NULL d_poses4x4, n_windows < 1, window_len
 * < 2, a stride outside [1, window_len - 1], a T_start that is not finite, and align_scale != 0 with
 * stride == window_len - 1 (no second frame shared); ORBX_ERR_UNSUPPORTED for more than 2^27 - 1 stream frames.  The
 * results go to a block of their own. */
int orbx_stitch_windows_device(orbx_ctx* ctx, const double* d_poses4x4, int n_windows, int window_len, int stride,
                               const double* T_start, int align_scale, void* stream);
/* Device-side view of the last stitch's results (src/with_bundle_adjustment.cpp:234-249: est_path), valid until the
 * next stitch; written on that call's stream. */
typedef struct {
  const double* trajectory4x4; /* [n_frames][16]: camera -> world, row-major */
  const int32_t* owner;        /* [n_frames]: the window the frame's pose was taken from */
  const double* anchors4x4;    /* [n_windows][16]: G(w), the stream pose of the window's first frame */
  const double* lambda;        /* [n_windows]: Lambda(w), the scale the window's translations were multiplied by */
  const int32_t* status;       /* [n_windows]: bits of orbx_st_status */
  int32_t n_frames, n_windows, window_len, stride;
} orbx_stitch_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before any stitch.  src/with_bundle_adjustment.cpp:234-249 */
int orbx_stitch_results_device(orbx_ctx* ctx, orbx_stitch_view* view);
/* Waits for the last stitch and copies stream frames [first_frame, first_frame + n_frames) and windows [first_window,
 * first_window + n_windows) in the view's layout (src/with_bundle_adjustment.cpp:234-249); every array may be NULL,
 * and a range whose arrays are all NULL is not checked. */
int orbx_stitch_fetch(orbx_ctx* ctx, int first_frame, int n_frames, double* trajectory4x4, int32_t* owner,
                      int first_window, int n_windows, double* anchors4x4, double* lambda, int32_t* status);
/* The same join on the host, no context: the same arithmetic from the same source
 * (src/with_bundle_adjustment.cpp:203, :234-249), the twin of orbx_chain_window_poses.  poses4x4: HOST; out:
 * trajectory4x4 (F x 16), owner (F), anchors4x4 (W x 16), lambda (W), status (W), each may be NULL.  Returns
 * ORBX_ERR_INVALID_ARG as orbx_stitch_windows_device does. */
int orbx_stitch_windows(const double* poses4x4, int n_windows, int window_len, int stride, const double* T_start,
                        int align_scale, double* trajectory4x4, int32_t* owner, double* anchors4x4, double* lambda,
                        int32_t* status);
/* The whole chain for a stream on DEVICE tracks, which may be the LK windows view
 * (src/with_bundle_adjustment.cpp:180-208, :234-249): orbx_tracks_pose_device, orbx_window_poses_stream_device, the
 * landmarks build (orbx_landmarks_build_chained_device for tri_mode ORBX_LM_TRI_FIRST_TWO with max_reproj_px == 0, else
 * orbx_landmarks_build_views_device on the chained poses), orbx_bundle_adjust_landmarks_device,
 * orbx_bundle_adjust_write_back_device and orbx_stitch_windows_device on the write-back's poses.  Asynchronous; nothing
 * is fetched.  Every stage's block is that stage's usual block, fetchable afterwards with the stage's own fetch.  An
 * argument any stage would refuse is refused before the first launch and leaves every previous block in place. */
int orbx_stream_odometry_tracks_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                       int n_windows, int slot_capacity, int window_len, int stride,
                                       const double* T_start, double scale0_first, double prob, double threshold,
                                       int pose_max_iters, uint64_t seed, int tri_mode, double max_reproj_px,
                                       double huber_delta, int ba_max_iters, double max_rot, double max_trans,
                                       int align_scale, void* stream);
/* Host convenience, the synchronous twin, modelled on orbx_window_odometry_tracks (include/orbx_vo.h;
 * src/with_bundle_adjustment.cpp:180-208, :234-249): HOST tracks (n_windows x n_slots x window_len x 2) and seen
 * (n_windows x n_slots) through orbx_stream_odometry_tracks_device on the context's stream.  Out: trajectory4x4 (F x 16), required;
 * st_status, wp_status, lm_status (n_windows each) and summaries (n_windows) may be NULL.  Replaces the results of all
 * six stages. */
int orbx_stream_odometry_tracks(orbx_ctx* ctx, const double* K, const float* tracks_xy, const int32_t* seen,
                                int n_windows, int n_slots, int window_len, int stride, const double* T_start,
                                double scale0_first, double prob, double threshold, int pose_max_iters, uint64_t seed,
                                int tri_mode, double max_reproj_px, double huber_delta, int ba_max_iters,
                                double max_rot, double max_trans, int align_scale, double* trajectory4x4,
                                int32_t* st_status, int32_t* wp_status, int32_t* lm_status,
                                orbx_ba_summary* summaries);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_STREAM_H */
