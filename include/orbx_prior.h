/* orbx_prior.h -- the eighth public header of liborbx.so: landmark priors in the window solve.
 *
 * The reference's problem is reprojection residuals with pose 0 constant (src/with_bundle_adjustment.cpp:612-679), so
 * its scale is free, and it keeps no point across a solve (src/with_bundle_adjustment.cpp:586-593).  A window carried
 * from the last generation (include/orbx_carry.h) is re-triangulated from its PnP poses; the solve then moves its
 * landmarks wherever reprojection is flat.  Here a landmark may carry an anchor and a weight, and the solve keeps it
 * near the coordinates it had on the map.  One generation of a carried stream, all on the device:
 *   orbx_landmarks_carry_device -> orbx_window_poses_pnp_carried_device -> orbx_landmarks_build_carried_device ->
 *   orbx_landmarks_priors_carried_device -> orbx_bundle_adjust_landmarks_prior_device -> the write-back, or the carry
 *   of the next generation with ORBX_CARRY_SOLVED.
 * Rules (rules 1-9 are rank 7's):
 *   P1 term   landmark j may carry an anchor A_j and a weight lambda_j >= 0.  lambda_j > 0 adds the residual block
 *             sqrt(lambda_j) (X_j - A_j), with no loss function: rho_j = lambda ((d0 d0 + d1 d1) + d2 d2), d = X - A; the
 *             diagonal of V_j gets + lambda and g_j gets + lambda d, AFTER the landmark's last observation.
 *             lambda_j = 0 is no operation at all: a problem whose weights are all 0 has every bit of the plain solve
 *   P2 cost   1/2 (sum rho_obs + sum rho_prior); a landmark's prior term sits right behind its observation terms in
 *             rule 9's lane order, in the linearisation and in the candidate alike.  initial_cost and final_cost of
 *             orbx_ba_summary include it
 *   P3 scales the Jacobi scales (rule 5) are taken from V including the prior
 *   P4        everything else is rank 7's: pose 0 constant, every landmark still needs an observation, the `failure`
 *             conditions, write-back only on convergence
 *   P5 start  ORBX_PRIOR_START_GIVEN: the points start as given or as built; ORBX_PRIOR_START_ANCHOR: every landmark
 *             with lambda_j > 0 starts at the bits of A_j.  On anything but convergence the returned blocks are the
 *             given ones
 *   P6 carried  for every ORBX_LM_OK window w of the current landmarks block and its landmark j with slot
 *             s = slot_of_point[j]: when the last carry block has point[w][s] >= 0, A_j = the bits of xyz[w][s] and
 *             lambda_j = weight; otherwise A_j = 0 and lambda_j = 0.  count[w] = the landmarks with a prior; a window that
 *             is not OK has count 0
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the blocks it reads when they were written on another stream.  On any error nothing is
 * launched or written, the previous results stay fetchable and the context usable. */
#ifndef ORBX_PRIOR_H
#define ORBX_PRIOR_H

#include "orbx.h"
#include "orbx_carry.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_PRIOR_START_GIVEN = 0, /* the points start as given (host entries) or as built (device entry) */
  ORBX_PRIOR_START_ANCHOR = 1 /* every landmark with a positive weight starts at its anchor */
} orbx_prior_start;

/* orbx_bundle_adjust (include/orbx.h) with landmark priors, where the reference's problem has reprojection residuals
 * only (src/with_bundle_adjustment.cpp:612-679): the same staging, workspaces and refusals.  prior_xyz (3 x n_points
 * doubles) and prior_weight (n_points doubles) may be NULL TOGETHER: no priors.  start: an orbx_prior_start.
 * ORBX_ERR_INVALID_ARG also for a negative or non-finite weight, a non-finite anchor under a positive weight, a start
 * that is neither value, and exactly one of the two arrays NULL. */
int orbx_bundle_adjust_prior(orbx_ctx* ctx, const double* K, int n_poses, double* poses6, int n_points, double* points3,
                             int n_obs, const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             const double* prior_xyz, const double* prior_weight, int start, double huber_delta,
                             int max_iters, orbx_ba_summary* summary);
/* orbx_bundle_adjust_batch (include/orbx.h) with landmark priors (src/with_bundle_adjustment.cpp:612-679): prior_xyz
 * and prior_weight run over all windows' landmarks in the order of points3.  Everything else as above. */
int orbx_bundle_adjust_prior_batch(orbx_ctx* ctx, const double* K, int n_windows, const int32_t* pose_offset,
                                   double* poses6, const int32_t* point_offset, double* points3,
                                   const int32_t* obs_offset, const int32_t* obs_point, const int32_t* obs_pose,
                                   const double* obs_xy, const double* prior_xyz, const double* prior_weight, int start,
                                   double huber_delta, int max_iters, orbx_ba_summary* summaries);
/* Rule P6 on the context's CURRENT landmarks block and its LAST carry block, where the reference keeps no point across
 * a solve (src/with_bundle_adjustment.cpp:586-593).  One weight per call.  The result is a block of its own, and it
 * remembers the landmarks block it was gathered for.  ORBX_ERR_INVALID_ARG: no carry block or no landmarks block, a
 * carry block whose n_windows or slot_capacity differs from the landmarks block's, a weight that is negative or not
 * finite. */
int orbx_landmarks_priors_carried_device(orbx_ctx* ctx, double weight, void* stream);
/* Device-side view of the last priors block, valid until the next one.  prior: anchor (3) and weight (1) of every
 * landmark in the landmarks block's point order (landmark j of window w at point_offset[w] + j).
 * src/with_bundle_adjustment.cpp:586-593 */
typedef struct {
  const double* prior;  /* [points][4] */
  const int32_t* count; /* [n_windows] */
  int32_t n_windows;
} orbx_landmarks_priors_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first priors block.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_priors_results_device(orbx_ctx* ctx, orbx_landmarks_priors_view* view);
/* Waits for the last priors block and copies windows [first, first + n): prior_xyz (3 per landmark) and prior_weight
 * (1 per landmark) in the format of orbx_bundle_adjust_prior_batch, count (n); each may be NULL.  *n_points (may be
 * NULL) = the landmarks of those windows; ORBX_ERR_CAPACITY when that is more than capacity and an array is asked for.
 * The block keeps the point offsets it was gathered with, so it stays fetchable after the landmarks block has been
 * rebuilt.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_priors_fetch(orbx_ctx* ctx, int first, int n, double* prior_xyz, double* prior_weight,
                                int32_t* count, int capacity, int* n_points);
/* orbx_bundle_adjust_landmarks_device (include/orbx.h) with the last priors block
 * (src/with_bundle_adjustment.cpp:612-679): it starts from the block's own poses and writes THE SAME solve state, so
 * orbx_bundle_adjust_landmarks_fetch, the write-back (include/orbx_vo.h) and ORBX_CARRY_SOLVED read it unchanged.
 * start: an orbx_prior_start.  ORBX_ERR_INVALID_ARG also without a priors block, when the landmarks block has been
 * rebuilt since the priors were gathered, and for a start that is neither value. */
int orbx_bundle_adjust_landmarks_prior_device(orbx_ctx* ctx, double huber_delta, int max_iters, int start, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PRIOR_H */
