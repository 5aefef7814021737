/* orbx_carry.h -- the sixth public header of liborbx.so: landmarks carried from one generation of tracked windows
 * into the next, and the next window localised against them by PnP.
 *
 * The reference re-detects its points from scratch at every solve (src/with_bundle_adjustment.cpp:586-593) and chains
 * cur_pose = prev_pose * T.inv() (src/with_bundle_adjustment.cpp:196-208), so every window has a metric frame of its
 * own.  Here window w of a call is stream w's CURRENT window and one call is one generation of many streams: the
 * top-up (orbx_good_features_topup_device, include/orbx.h) hands the live tracks of a window's last frame to the next
 * window with `origin`, the slot each came from; the carry joins origin to the old window's landmarks, the carried PnP
 * localises EVERY frame of the new window, frames 0 and 1 included, against those landmarks, and the carried build
 * triangulates the new window's landmarks from those poses.  The map keeps one frame and one scale from window to
 * window with no scale ratio involved.  One generation, all on the device:
 *   landmarks block of generation g (built, optionally solved)  ->  top-up  ->  orbx_lk_track_windows[_fb]_device  ->
 *   orbx_landmarks_carry_device  ->  orbx_window_poses_pnp_carried_device  ->  orbx_landmarks_build_carried_device  ->
 *   orbx_bundle_adjust_landmarks_device, the write-back ... as before.
 * Rules:
 *   A carry    new slot s of window w is carried iff the old status[w] is ORBX_LM_OK, o = origin[w][s] lies in
 *              [0, old slot_capacity), a landmark j of old window w has slot_of_point == o (at most one: the slots of a
 *              window ascend) and its three source doubles are finite.  The carry block holds xyz[w][s] (the doubles,
 *              bits unchanged), point[w][s] = j (-1 when not carried; xyz is 0 then) and count[w].  Two new slots with
 *              the same origin are both carried
 *   B gather   problem (w, k), k = 0 .. window_len - 1, takes in ascending slot order every carried slot s with
 *              seen[w][s] (clamped to [0, window_len]) > k and both floats of tracks_xy[w][s][k] finite; the pixel is
 *              widened to double
 *   C solve    the rules of include/orbx_pnp.h from `sample` to `result`; the seed of problem (w, k) is
 *              mix64(seed ^ mix64(k)), so frames k >= 2 sample as orbx_window_poses_pnp_device samples them and a
 *              window's result does not depend on its place in the batch.  The mask is indexed by SLOT
 *   D status   ORBX_PNP_SKIPPED iff count[w] == 0; ORBX_PNP_FEW_POINTS and ORBX_PNP_NO_MODEL as in include/orbx_pnp.h.
 *              A record that is not ORBX_PNP_OK has pose6 = zeros, inliers = 0 and rms_px = 0
 *   E fill     window_status[w] is ORBX_CARRY_LOST iff problem (w, 0) or (w, 1) is not ORBX_PNP_OK.  poses6[w][k] of
 *              an ORBX_CARRY_OK window is the record's pose where the record is OK, otherwise (k >= 2) the bytes of
 *              poses6[w][k - 1]: the camera stays where it was.  A LOST window has all zeros
 *   F build    orbx_landmarks_build_device with the poses read from the carried-PnP block on the device; a LOST window
 *              becomes ORBX_LM_BAD_POSE and owns no landmark
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the blocks it reads when they were written on another stream.  On any error nothing is
 * launched or written, the previous results stay fetchable and the context usable. */
#ifndef ORBX_CARRY_H
#define ORBX_CARRY_H

#include "orbx.h"
#include "orbx_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_CARRY_BUILT = 0, /* the landmarks block's points3 as built */
  ORBX_CARRY_SOLVED = 1 /* the point array of the last solve of this block (orbx_bundle_adjust_landmarks_fetch's) */
} orbx_carry_source;

typedef enum {
  ORBX_CARRY_OK = 0,
  ORBX_CARRY_LOST = 1 /* frame 0 or frame 1 could not be localised: the caller re-initialises the stream */
} orbx_carry_status;

/* Rule A on the context's CURRENT landmarks block (the "old" one); the reference keeps no point across a solve, it
 * re-detects (src/with_bundle_adjustment.cpp:586-593).  d_origin: device int32 [n_windows][slot_capacity], e.g. the
 * top-up view's origin; slot_capacity is the NEW windows' capacity.  source: an orbx_carry_source; after
 * ORBX_BA_NO_CONVERGENCE a solve leaves its blocks unchanged, so ORBX_CARRY_SOLVED needs no termination test.  The
 * result is a block of its own: it survives the next landmarks build, and every other block stays as it is.
 * ORBX_ERR_INVALID_ARG: d_origin NULL, no landmarks block, n_windows other than the block's, slot_capacity < 1, a source
 * that is neither, ORBX_CARRY_SOLVED on a block that has not been solved; ORBX_ERR_UNSUPPORTED: slot_capacity above
 * 65536 or more slots in the batch than 32-bit offsets hold. */
int orbx_landmarks_carry_device(orbx_ctx* ctx, const int32_t* d_origin, int n_windows, int slot_capacity, int source,
                                void* stream);
/* Device-side view of the last carry, valid until the next one.  Slots that are not carried hold xyz = 0 and
 * point = -1, so whole arrays compare equal.  src/with_bundle_adjustment.cpp:586-593 */
typedef struct {
  const double* xyz;    /* [n_windows][slot_capacity][3] */
  const int32_t* point; /* [n_windows][slot_capacity]: the landmark's index inside the old window, or -1 */
  const int32_t* count; /* [n_windows] */
  int32_t slot_capacity, n_windows;
} orbx_landmarks_carry_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first carry.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_carry_results_device(orbx_ctx* ctx, orbx_landmarks_carry_view* view);
/* Waits for the last carry and copies windows [first, first + n): xyz (n x slot_capacity x 3), point
 * (n x slot_capacity), count (n); each may be NULL.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_landmarks_carry_fetch(orbx_ctx* ctx, int first, int n, double* xyz, int32_t* point, int32_t* count);
/* Rules B to E: every (window, frame k >= 0) of the new windows' tracks against the last carry block, where the
 * reference chains (src/with_bundle_adjustment.cpp:196-208).  d_tracks_xy / d_seen: the layout of
 * orbx_lk_windows_view.  The argument rules of orbx_pnp_ransac apply; ORBX_ERR_INVALID_ARG also when there is no carry
 * block, n_windows or slot_capacity differs from the carry block's, or window_len is outside [2, ORBX_BA_MAX_POSES]. */
int orbx_window_poses_pnp_carried_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy,
                                         const int32_t* d_seen, int n_windows, int slot_capacity, int window_len,
                                         double prob, double threshold_px, int max_iters, uint64_t seed,
                                         int refine_iters, int min_inliers, void* stream);
/* Device-side view of the last orbx_window_poses_pnp_carried_device, valid until the next one.  Problem (w, k) is
 * record w * window_len + k.  mask: indexed by slot.  window_status: an orbx_carry_status per window.
 * src/with_bundle_adjustment.cpp:196-208 */
typedef struct {
  const orbx_pnp_record* records; /* [n_windows][window_len] */
  const double* poses6;           /* [n_windows][window_len][6] */
  const uint8_t* mask;            /* [n_windows][window_len][slot_capacity] */
  const int32_t* window_status;   /* [n_windows] */
  int32_t slot_capacity, window_len, n_windows;
} orbx_window_poses_carried_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first batch.  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_carried_results_device(orbx_ctx* ctx, orbx_window_poses_carried_view* view);
/* Waits for the last batch and copies windows [first, first + n): records (n x window_len), poses6
 * (n x window_len x 6) and window_status (n); each may be NULL.  src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_carried_fetch(orbx_ctx* ctx, int first, int n, orbx_pnp_record* records, double* poses6,
                                        int32_t* window_status);
/* The mask of problem (window, k), k in [0, window_len): one byte per slot, *count = slot_capacity;
 * ORBX_ERR_CAPACITY if that is more than capacity (count is still written).
 * src/with_bundle_adjustment.cpp:196-208 */
int orbx_window_poses_pnp_carried_mask_fetch(orbx_ctx* ctx, int window, int k, uint8_t* mask, int capacity,
                                             int* count);
/* Rule F: orbx_landmarks_build_device (include/orbx.h) with the poses read from the last carried-PnP block on the
 * device, where the reference builds from its chained poses (src/with_bundle_adjustment.cpp:196-208).  n_windows and
 * window_len must be that block's (ORBX_ERR_INVALID_ARG otherwise, and before the first carried PnP); every other rule
 * is the build's.  An ORBX_CARRY_LOST window becomes ORBX_LM_BAD_POSE, as orbx_landmarks_build_chained_device treats
 * ORBX_WP_NONFINITE.  The result IS the landmarks block: every orbx_landmarks_* and orbx_bundle_adjust_landmarks_*
 * entry and the write-back work on it unchanged. */
int orbx_landmarks_build_carried_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                        int n_windows, int slot_capacity, int window_len, void* stream);
/* Carry and carried PnP of ONE window on HOST arrays, synchronous, where the reference re-detects and chains
 * (src/with_bundle_adjustment.cpp:586-593, src/with_bundle_adjustment.cpp:196-208).  old_points3 (n_old x 3 doubles)
 * and old_slot_of_point (n_old, ascending) are an old window's landmarks as fetched; origin, seen (n_slots each) and
 * tracks_xy (n_slots x window_len x 2 floats) are the new window; an origin is in range when it is >= 0.  Outputs, each
 * may be NULL: records (window_len), poses6 (window_len x 6), window_status (one orbx_carry_status), carried_point
 * (n_slots: rule A's point).  It runs as a carry and a carried PnP of one window and replaces those two blocks only.
 * ORBX_ERR_INVALID_ARG (nothing is launched, no output is written): the cases of orbx_pnp_ransac, n_old < 0,
 * n_slots < 1, window_len outside [2, ORBX_BA_MAX_POSES], a NULL origin, tracks_xy or seen, old_points3 or
 * old_slot_of_point NULL with n_old > 0; ORBX_ERR_UNSUPPORTED: n_old or n_slots above 65536. */
int orbx_localise_carried_window(orbx_ctx* ctx, const double* old_points3, const int32_t* old_slot_of_point, int n_old,
                                 const int32_t* origin, const float* tracks_xy, const int32_t* seen, int n_slots,
                                 int window_len, const double* K, double prob, double threshold_px, int max_iters,
                                 uint64_t seed, int refine_iters, int min_inliers, orbx_pnp_record* records,
                                 double* poses6, int32_t* window_status, int32_t* carried_point);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_CARRY_H */
