/* orbx_search.h -- the ninth public header of liborbx.so: the search by projection.  The
 * landmarks of the current block projected into a predicted view, and two described point sets re-associated inside a
 * position gate around those predictions.
 *
 * Ranks 17 to 20 keep a map from window to window; rank 19 joins a window to it by descriptor alone
 * (orbx_reassociate_device, include/orbx_reloc.h), as the reference's only matcher does
 * (src/feature_tracking.cpp:203-219): every query against every train slot, and a ratio test that two map points which
 * look alike fail even when they lie far apart in the image.  The reference keeps no point across a solve
 * (src/with_bundle_adjustment.cpp:586-593), so it has no prediction to gate with; here the block holds the old
 * window's landmarks and its last pose:
 *   orbx_landmarks_project_device(the carried PnP's last pose, read in place) -> view.xy / view.state, by OLD SLOT
 *   orbx_reassociate_gated_device(query = bank 1 with its points, train = bank 0 with view.xy / view.state)
 *   -> orbx_reassociate_results_device's origin -> orbx_landmarks_carry_device -> ... as in include/orbx_carry.h.
 * Rules:
 *   P1 landmark old slot t of window w has a landmark iff rule A of the carry would carry origin t: the window is
 *               ORBX_LM_OK, a landmark j has slot_of_point == t, and its three source doubles are finite.  Otherwise the
 *               slot is ORBX_PROJ_NONE
 *   P2 pose     the predicted pose (angle-axis and translation, world -> camera) is prepared by ba_pose_prepare; one
 *               that is not finite or beyond BA_MAX_THETA is not accepted: every slot of the window is ORBX_PROJ_NONE and
 *               count[w] = 0
 *   P3 point    p = R X + t with the three sums of the PnP score (pnp_inlier), in its association order; the slot is
 *               ORBX_PROJ_BEHIND iff !(p2 > 0)
 *   P4 pixel    u = fx * p0 / p2 + cx, v = fy * p1 / p2 + cy, evaluated as the PnP score evaluates them: a landmark's
 *               predicted pixel under a PnP pose is bit for bit the pixel PnP scored.  depth = p2
 *   P5 state    ORBX_PROJ_OK iff u and v are finite, -margin_px <= u <= width - 1 + margin_px and -margin_px <= v <=
 *               height - 1 + margin_px, otherwise ORBX_PROJ_OUTSIDE.  A slot that is not OK holds zeros in xy and depth;
 *               count[w] counts the OK slots.  Whole arrays compare equal
 *   F sets      (rank 19) only ORBX_PD_OK slots take part, on both sides
 *   K positioned a train slot is positioned iff its pstate is ORBX_PROJ_OK (or no pstate is given) and both doubles are
 *               finite; a query is positioned iff both floats are finite
 *   L gate      train slot t is a candidate of query q iff both are ORBX_PD_OK, both are positioned and dx * dx + dy *
 *               dy <= radius_px * radius_px with dx = (double)qx - tx, dy = (double)qy - ty, every product and sum
 *               rounded once and nothing contracted; a pair exactly on the circle is a candidate.  candidates[w][q]
 *               counts them, 0 for a query that is not OK or not positioned
 *   M 2-NN      the best and the second-best CANDIDATE by Hamming distance, ties to the lower train slot: the two
 *               smallest keys (d << 22) | t, whatever the order the candidates are visited in
 *   N accept    two candidates or more: rule H of rank 19 -- (double)(float)d1 < ratio * (double)(float)d2 and d1 <=
 *               max_distance.  Exactly one: accepted iff accept_lone == 1 and d1 <= max_distance
 *   I, J        (rank 19) unchanged, on the same keys
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL.  The
 * projection waits on the device for the landmarks block and its solve, the carried PnP and the window poses (its
 * poses may be theirs); the gated re-association for the projection, the descriptor banks, the good-features, top-up
 * and windows-tracker blocks; orbx_landmarks_carry_device waits for the re-association block the gated call writes.
 * On any error nothing is launched or written, the previous results stay fetchable and the context usable.  A call
 * reads the caller's arrays while it runs: a producer that replaces them on ANOTHER stream has to be ordered behind it
 * by the caller.
 * Not here: levels other than 0, a gate from a depth or scale prediction (the radius is one number), refreshing a
 * landmark's descriptor, choosing the prediction (the caller passes a pose); no stream entry calls the gate. */
#ifndef ORBX_SEARCH_H
#define ORBX_SEARCH_H

#include "orbx.h"
#include "orbx_carry.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_PROJ_NONE = 0,    /* no landmark (rule P1), or the window's pose was not accepted (rule P2) */
  ORBX_PROJ_BEHIND = 1,  /* !(depth > 0) (rule P3) */
  ORBX_PROJ_OUTSIDE = 2, /* beyond the frame grown by the margin, or not finite (rule P5) */
  ORBX_PROJ_OK = 3       /* xy and depth are the prediction */
} orbx_proj_state;

/* Rules P1 to P5 on the context's CURRENT landmarks block, where the reference keeps no point to project
 * (src/with_bundle_adjustment.cpp:586-593).  K: row-major 3x3 on the host.  The predicted pose of window w is the six
 * doubles at d_pose6 + w * pose_stride on the device (stride in doubles): the last pose of the carried-PnP view is
 * poses6 + 6 * (window_len - 1) with stride 6 * window_len.  source: an orbx_carry_source, with the carry's rule for
 * ORBX_CARRY_SOLVED.  The result is a block of its own, indexed by OLD SLOT -- the index the carry's origin names --
 * and every other block stays as it is.  ORBX_ERR_INVALID_ARG: K or d_pose6 NULL, a K whose focal lengths are not
 * positive or that is not finite, d_pose6 not 8-byte aligned, pose_stride < 6, no landmarks block, n_windows other
 * than the block's, a source that is neither, ORBX_CARRY_SOLVED on a block that has not been solved, width or height
 * < 1, a margin_px that is negative or not finite. */
int orbx_landmarks_project_device(orbx_ctx* ctx, const double* K, const double* d_pose6, size_t pose_stride,
                                  int n_windows, int source, int width, int height, double margin_px, void* stream);
/* Device-side view of the last projection, valid until the next one.  xy and state have the shape
 * orbx_reassociate_gated_device takes as d_train_xy and d_train_pstate (t_capacity = slot_capacity).  Slots that are
 * not ORBX_PROJ_OK hold zeros.  src/with_bundle_adjustment.cpp:586-593 */
typedef struct {
  const double* xy;     /* [n_windows][slot_capacity][2]: the predicted pixel */
  const double* depth;  /* [n_windows][slot_capacity] */
  const int32_t* state; /* [n_windows][slot_capacity]: an orbx_proj_state */
  const int32_t* count; /* [n_windows]: the ORBX_PROJ_OK slots */
  int32_t slot_capacity, n_windows;
} orbx_landmarks_projection_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first projection.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_project_results_device(orbx_ctx* ctx, orbx_landmarks_projection_view* view);
/* Waits for the last projection and copies windows [first, first + n): xy (n x slot_capacity x 2), depth, state
 * (n x slot_capacity each) and count (n); each may be NULL.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_project_fetch(orbx_ctx* ctx, int first, int n, double* xy, double* depth, int32_t* state,
                                 int32_t* count);
/* Rules P1 to P5 for ONE old window on HOST arrays, synchronous, as orbx_localise_carried_window takes an old window:
 * points3 (n_old x 3) and the ascending slot_of_point (n_old), a window that is ORBX_LM_OK; pose6: six host doubles.
 * Outputs xy (slot_capacity x 2), depth, state (slot_capacity each) and count (one); each may be NULL.  It runs as a
 * projection of one window and replaces that block.  ORBX_ERR_INVALID_ARG: n_old < 0, a NULL input with a positive
 * size, pose6 NULL, slot_capacity < 1 and the parameter cases of orbx_landmarks_project_device; ORBX_ERR_UNSUPPORTED:
 * n_old or slot_capacity above 65536.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_project_landmarks(orbx_ctx* ctx, const double* points3, const int32_t* slot_of_point, int n_old,
                           int slot_capacity, const double* K, const double* pose6, int width, int height,
                           double margin_px, double* xy, double* depth, int32_t* state, int32_t* count);

/* Rules F, K to N, I and J for n_windows pairs of described sets with positions, where the reference matches two ORB
 * sets without geometry (src/feature_tracking.cpp:203-219).  desc / state: exactly what orbx_reassociate_device takes.
 * The query positions are a strided float source, as orbx_describe_points_device takes its points: slot q of window w
 * is the two floats at d_query_xy + w * xy_frame_stride + q * point_stride (strides in floats).  d_train_xy: double
 * [n_windows][t_capacity][2]; d_train_pstate: int32 [n_windows][t_capacity], an orbx_proj_state per slot, or NULL:
 * every slot is positioned.  The projection view is one valid source, any caller-held prediction another.  The call
 * REPLACES the context's re-association block: orbx_reassociate_results_device / _fetch serve it, and
 * orbx_landmarks_carry_device waits for it.  candidates is a block of its own.  ORBX_ERR_INVALID_ARG: the cases of
 * orbx_reassociate_device, d_query_xy NULL or not 4-byte aligned, point_stride < 2 or xy_frame_stride < point_stride *
 * (q_capacity - 1) + 2, d_train_xy NULL or not 8-byte aligned, d_train_pstate not 4-byte aligned, a radius_px that is
 * not finite or not > 0, accept_lone outside {0, 1}; ORBX_ERR_UNSUPPORTED: as orbx_reassociate_device. */
int orbx_reassociate_gated_device(orbx_ctx* ctx, const orbx_descriptor* d_query_desc, const int32_t* d_query_state,
                                  const float* d_query_xy, size_t point_stride, size_t xy_frame_stride, int q_capacity,
                                  const orbx_descriptor* d_train_desc, const int32_t* d_train_state,
                                  const double* d_train_xy, const int32_t* d_train_pstate, int t_capacity,
                                  int n_windows, double radius_px, double ratio, int max_distance, int accept_lone,
                                  int unique, void* stream);
/* Device-side view of the candidates of the last gated re-association, valid until the next one.
 * src/feature_tracking.cpp:203-219 */
typedef struct {
  const int32_t* candidates; /* [n_windows][q_capacity]: the train slots inside the query's gate (rule L) */
  int32_t q_capacity, n_windows;
} orbx_reassociate_gated_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first gated re-association.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate_gated_results_device(orbx_ctx* ctx, orbx_reassociate_gated_view* view);
/* Waits for the last gated re-association and copies candidates of windows [first, first + n) (n x q_capacity); it
 * may be NULL.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate_gated_fetch(orbx_ctx* ctx, int first, int n, int32_t* candidates);
/* The same rules for ONE window on HOST arrays, synchronous: query_xy (nq x 2 floats), train_xy (nt x 2 doubles),
 * train_pstate (nt, or NULL); outputs origin, dist, candidates (nq each) and count (one), each may be NULL.  It runs as
 * a gated re-association of one window and replaces those blocks.  nq == 0 writes count = 0 and launches nothing.
 * ORBX_ERR_INVALID_ARG: nq < 0, nt < 0, a NULL input with a positive size (train_pstate excepted), and the parameter
 * cases of orbx_reassociate_gated_device.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate_gated(orbx_ctx* ctx, const orbx_descriptor* query_desc, const int32_t* query_state,
                           const float* query_xy, int nq, const orbx_descriptor* train_desc,
                           const int32_t* train_state, const double* train_xy, const int32_t* train_pstate, int nt,
                           double radius_px, double ratio, int max_distance, int accept_lone, int unique,
                           int32_t* origin, int32_t* dist, int32_t* count, int32_t* candidates);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_SEARCH_H */
