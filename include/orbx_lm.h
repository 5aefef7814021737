/* orbx_lm.h -- the third public header of liborbx.so: the landmarks block of tracked windows built from every view of a
 * track, with a reprojection gate and per-slot diagnostics.
 *
 * The reference's buildLandmarksFromFirstTwoFramesAndTracks (src/with_bundle_adjustment.cpp:502-575) triangulates every
 * track from frames 0 and 1, the shortest baseline of the window, and checks z > 0 in WORLD coordinates only.  The
 * entries here choose per call
 *   tri_mode       the views the point is triangulated from: the first two (the reference), the first and the last one
 *                  the track was seen in, or every one it was seen in
 *   max_reproj_px  0, or the largest reprojection error in pixels over the observed views that a landmark may have
 * and write THE SAME landmarks block: orbx_landmarks_results_device / _fetch, orbx_bundle_adjust_landmarks_device /
 * _fetch (include/orbx.h) and orbx_bundle_adjust_write_back_device (include/orbx_vo.h) work on it unchanged.
 * Rules (csrc/orbx_lm_math.h holds the arithmetic, tests/cpp/lm_views_sequential.cpp restates the
 * kernels sequentially and results are bit-identical to it), with sn = seen clamped into [0, window_len]:
 *   window   the baseline gate of orbx_landmarks_build_device on poses 0 and 1 in every mode.  With
 *            ORBX_LM_TRI_FIRST_TWO and max_reproj_px == 0 only poses 0 and 1 are prepared; otherwise every pose of the
 *            window is, and one whose rotation angle is beyond 1e5 rad makes the window ORBX_LM_BAD_POSE
 *   views    FIRST_TWO {0, 1}, WIDEST {0, sn - 1}, ALL_VIEWS {0 .. sn - 1}; sn < 2: ORBX_LM_SHORT
 *   system   two rows per view in ascending view order, the normal matrix summed row by row, the Jacobi sweeps of the
 *            two-view DLT; a slot with sn == 2 has the same point in all three modes, bit for bit
 *   point    X = h / h[3] in binary64; h[3] == 0 or a quotient that is not finite: ORBX_LM_DEGENERATE
 *   depth    FIRST_TWO keeps the reference's world z > 0; the other modes want the camera depth (R_k X + t_k).z > 0 in
 *            every observed view, else ORBX_LM_BEHIND
 *   gate     reproj_px = the largest distance in pixels between an observation and the projection of X over the
 *            observed views (+inf when one is not finite); with max_reproj_px > 0 a landmark beyond it is
 *            ORBX_LM_REPROJECTION.  (The observed views are those among the prepared ones.)
 * A landmark is rejected whole: its track is never trimmed.  Every device entry is asynchronous on the context's
 * stream, or on `stream` (a hipStream_t) when that is not NULL.  On any error nothing is launched or written, the
 * previous results stay fetchable and the context usable. */
#ifndef ORBX_LM_H
#define ORBX_LM_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { ORBX_LM_TRI_FIRST_TWO = 0, ORBX_LM_TRI_WIDEST = 1, ORBX_LM_TRI_ALL_VIEWS = 2 } orbx_lm_tri_mode;
typedef enum {
  ORBX_LM_KEPT = 0,
  ORBX_LM_SHORT = 1,        /* seen < 2 */
  ORBX_LM_DEGENERATE = 2,   /* h[3] == 0 or a quotient that is not finite */
  ORBX_LM_BEHIND = 3,       /* the depth check of the mode failed            src/with_bundle_adjustment.cpp:558-559 */
  ORBX_LM_REPROJECTION = 4, /* reproj_px beyond max_reproj_px */
  ORBX_LM_NO_WINDOW = 5     /* the window is not ORBX_LM_OK by its gate */
} orbx_lm_reason;

/* orbx_landmarks_build_device and orbx_landmarks_build_chained_device in one entry, with the two options
 * (src/with_bundle_adjustment.cpp:502-575).  poses6: HOST n_windows x window_len x 6, or NULL: the last window-poses
 * block (orbx_window_poses_device), whose n_windows / window_len must match.  tri_mode: an orbx_lm_tri_mode;
 * max_reproj_px: 0 = no gate.  Every refusal of those two entries applies; ORBX_ERR_INVALID_ARG also for a tri_mode
 * outside 0 .. 2 and a max_reproj_px that is negative or not finite.  The result is the landmarks block; reason and
 * reproj_px of every slot go to a buffer of their own. */
int orbx_landmarks_build_views_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                      int n_windows, int slot_capacity, int window_len, const double* poses6,
                                      int tri_mode, double max_reproj_px, void* stream);
/* Device-side view of the diagnostics of the last views build (src/with_bundle_adjustment.cpp:502-575), valid until
 * the next views build; a build by orbx_landmarks_build_device or orbx_landmarks_build_chained_device invalidates
 * them.  reproj_px is 0 where reason is ORBX_LM_SHORT, ORBX_LM_DEGENERATE or ORBX_LM_NO_WINDOW. */
typedef struct {
  const uint8_t* reason;  /* [n_windows][slot_capacity] orbx_lm_reason */
  const float* reproj_px; /* [n_windows][slot_capacity] */
  int32_t slot_capacity, n_windows;
} orbx_landmarks_views_view;
/* Fills the view; ORBX_ERR_INVALID_ARG unless the last landmarks build was a views build.
 * src/with_bundle_adjustment.cpp:502-575 */
int orbx_landmarks_views_results_device(orbx_ctx* ctx, orbx_landmarks_views_view* view);
/* Waits for the last views build and copies windows [first, first + n) in the view's layout; each array may be NULL.
 * src/with_bundle_adjustment.cpp:502-575 */
int orbx_landmarks_views_fetch(orbx_ctx* ctx, int first, int n, uint8_t* reason, float* reproj_px);
/* orbx_bundle_adjust_tracks with the two options: ONE window of host tracks through the views build and the solve as a
 * batch of one; every argument before tri_mode is orbx_bundle_adjust_tracks's.
 * src/with_bundle_adjustment.cpp:502-575, src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_tracks_views(orbx_ctx* ctx, const double* K, const float* tracks_xy, const int32_t* seen,
                                    int n_slots, int window_len, double* poses6, double huber_delta, int max_iters,
                                    int32_t* lm_status, orbx_ba_summary* summary, double* points3,
                                    int32_t* slot_of_point, int capacity, int* count, int tri_mode,
                                    double max_reproj_px);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_LM_H */
