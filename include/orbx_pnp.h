/* orbx_pnp.h -- the fifth public header of liborbx.so: perspective-n-point with RANSAC, batched over the later frames
 * of tracked windows.
 *
 * cv::solvePnPRansac in the reference's vocabulary.  The reference calls none: every pose it hands to its solve comes
 * from the chain cur_pose = prev_pose * T.inv() (src/with_bundle_adjustment.cpp:196-208), whose steps take their length
 * from get_scale's median ratio.  The landmarks of a window are triangulated from frames 0 and 1 (or from every view,
 * include/orbx_lm.h) and frames 2 .. window_len - 1 observe the same landmarks, so each later frame can be localised
 * against them in the landmarks' own metric frame, with no scale ratio involved.
 * Rules (csrc/orbx_pnp_math.h holds the arithmetic, tests/cpp/pnp_sequential.cpp restates the
 * kernel sequentially and results are bit-identical to it):
 *   gather    problem (window w, frame k >= 2) takes point j of window w iff rows[j] + k < rows[j + 1], in ascending j:
 *             the pixel is obs_xy at that row position, the world point is points3 as built
 *   sample    three distinct correspondences from (seed, iteration, n) by orbx_estimate_pose's counter hash and
 *             rejection rule; the seed of problem (w, k) of a batch is mix64(seed ^ mix64(k)) with that hash's
 *             mix64: the same for every window, so a window's result does not depend on its place in the batch
 *   solve     P3P: Grunert's distance equations reduced to one quartic, positive roots only, up to four (R, t) world ->
 *             camera in ascending root order
 *   score     inlier iff the camera depth is > 0 and the squared reprojection error in pixels is <= threshold_px^2
 *   select    in (iteration, model) order; a model becomes the best one iff it has more inliers than the best so far
 *             and at least min_inliers; the iteration count follows RANSACUpdateNumIters with exponent 3
 *   refine    at most refine_iters Levenberg-Marquardt steps on (angle-axis, t) over the best model's inliers, squared
 *             loss; the refined pose replaces the RANSAC pose only if its inlier count is not smaller
 *   result    mask, inliers and rms_px come from the pose that is kept
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the landmarks block when that was written on another stream.  On any error nothing is
 * launched or written, the previous results stay fetchable and the context usable. */
#ifndef ORBX_PNP_H
#define ORBX_PNP_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_PNP_OK = 0,
  ORBX_PNP_SKIPPED = 1,    /* the window is not ORBX_LM_OK */
  ORBX_PNP_FEW_POINTS = 2, /* fewer than min_inliers correspondences */
  ORBX_PNP_NO_MODEL = 3    /* no model reached min_inliers */
} orbx_pnp_status;

#define ORBX_PNP_MAX_REFINE_ITERS 20

/* One problem's result.  pose6: angle-axis and translation, world -> camera, of the pose that is kept; with a status
 * other than ORBX_PNP_OK the pose the landmarks block was built with (zeros from orbx_pnp_ransac), inliers = 0 and
 * rms_px = 0.  iters: RANSAC iterations run; n_corr: correspondences gathered; rms_px: the root of the mean squared
 * reprojection error of the inliers.  src/with_bundle_adjustment.cpp:196-208 */
typedef struct {
  double pose6[6];
  int32_t inliers, iters, n_corr, status;
  double rms_px;
} orbx_pnp_record;

/* solvePnPRansac on HOST arrays, a batch of one, synchronous (src/with_bundle_adjustment.cpp:196-208 is what it
 * stands beside).  points3: n x 3 doubles, world; pixels_xy: n x 2 doubles; K: row-major double[9].  `seed` is the
 * problem's own seed.  Outputs, each may be NULL: pose6 (6 doubles), mask (n bytes), inliers, iters, rms_px, status
 * (an orbx_pnp_status; ORBX_PNP_SKIPPED does not occur).  ORBX_ERR_INVALID_ARG (nothing is launched, no output is
 * written): the cases of orbx_estimate_pose -- K NULL or with a non-finite fx, fy, cx or cy, fx <= 0 or fy <= 0, a
 * non-finite prob (a finite one is clamped to [0, 1]), a threshold_px that is negative or not finite, max_iters
 * outside [0, ORBX_POSE_MAX_ITERS], n < 0 -- and refine_iters outside [0, ORBX_PNP_MAX_REFINE_ITERS], min_inliers < 4,
 * points3 or pixels_xy NULL with n > 0. */
int orbx_pnp_ransac(orbx_ctx* ctx, const double* points3, const double* pixels_xy, int n, const double* K, double prob,
                    double threshold_px, int max_iters, uint64_t seed, int refine_iters, int min_inliers,
                    double* pose6, uint8_t* mask, int32_t* inliers, int32_t* iters, double* rms_px, int32_t* status);
/* Every (window, frame >= 2) of the LAST landmarks block against that block's landmarks, with the K the block was
 * built with; the reference chains these poses instead (src/with_bundle_adjustment.cpp:196-208).  The argument rules
 * of orbx_pnp_ransac apply; ORBX_ERR_INVALID_ARG also when no landmarks block has been built or its window_len is 2. */
int orbx_window_poses_pnp_device(orbx_ctx* ctx, double prob, double threshold_px, int max_iters, uint64_t seed,
                                 int refine_iters, int min_inliers, void* stream);
/* Device-side view of the last orbx_window_poses_pnp_device, valid until the next one.  Problem (w, k) is record
 * w * (window_len - 2) + k - 2.  poses6: the SEEDED poses: frames 0 and 1 are the block's built poses, frame k holds
 * the PnP pose when its status is ORBX_PNP_OK and otherwise the built pose.  mask: indexed by the point's index inside
 * its window.  src/with_bundle_adjustment.cpp:196-208 */
typedef struct {
  const orbx_pnp_record* records; /* [n_windows][window_len - 2] */
  const double* poses6;           /* [n_windows][window_len][6] */
  const uint8_t* mask;            /* [n_windows][window_len - 2][slot_capacity] */
  int32_t slot_capacity, window_len, n_windows;
} orbx_window_poses_pnp_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first batch.  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_results_device(orbx_ctx* ctx, orbx_window_poses_pnp_view* view);
/* Waits for the last batch and copies windows [first, first + n): records (n x (window_len - 2)) and seeded poses6
 * (n x window_len x 6); each may be NULL.  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_fetch(orbx_ctx* ctx, int first, int n, orbx_pnp_record* records, double* poses6);
/* The mask of problem (window, k): one byte per point of the window, *count = the window's points;
 * ORBX_ERR_CAPACITY if that is more than capacity (count is still written).  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_mask_fetch(orbx_ctx* ctx, int window, int k, uint8_t* mask, int capacity, int* count);
/* orbx_bundle_adjust_landmarks_device (include/orbx.h) with the solve's poses copy taken from the SEEDED poses of the
 * last orbx_window_poses_pnp_device, which must belong to the current landmarks block (ORBX_ERR_INVALID_ARG
 * otherwise).  The landmarks block itself stays as built: orbx_bundle_adjust_landmarks_fetch reads the result as
 * before, and the write-back gate (orbx_bundle_adjust_write_back_device) still compares the solved poses against the
 * poses the block was BUILT with, not against the seeds.  src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_landmarks_pnp_device(orbx_ctx* ctx, double huber_delta, int max_iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PNP_H */
