/* orbx_reloc.h -- the seventh public header of liborbx.so: ORB descriptors at points the caller already holds, and two
 * described point sets joined into the `origin` block that the landmarks carry reads.
 *
 * Ranks 17 and 18 keep a map from window to window, but the only bridge between two windows is the top-up's `origin`,
 * and only Lucas-Kanade tracking produces one: after a frame gap, a large motion or an ORBX_CARRY_LOST the map cannot
 * be reached.  The reference falls back to ORB plus the matcher when fewer than 150 tracks survive
 * (src/feature_tracking.cpp:68-71, the matcher at src/feature_tracking.cpp:203-219).  Here the device half of that
 * fallback: a window that lost its tracks detects fresh corners, describes them, and is re-associated to the old
 * window's slots by descriptor; the existing carry -> carried PnP -> carried build continue in the old metric frame:
 *   old window's last frame:  points (LK view, top-up view or good-features view) -> orbx_describe_points_device, bank 0
 *   new window's first frame: orbx_good_features_batch_device -> orbx_describe_points_device, bank 1
 *   orbx_reassociate_device(query = bank 1, train = bank 0) -> view.origin -> orbx_landmarks_carry_device -> ... as in
 *   include/orbx_carry.h.
 * Rules:
 *   A live      slot s of frame f is live iff s < counts[f] (when counts is given) and seen[f][s] >= seen_min (when
 *               seen is given).  It is usable iff both floats are finite, 0 <= x <= width - 1 and 0 <= y <= height - 1
 *               by float compares
 *   B pixel     X = (int)rintf(x), Y = (int)rintf(y): ties to even (20.5 -> 20, 21.5 -> 22)
 *   C interior  R = max(patch_size / 2, 20).  The 20 is the BRIEF pattern's reach: the largest hypot of a pattern point
 *               is 18.38, so a rotated and rounded offset is at most 18, plus 2 for the 5x5 box.  A usable slot is
 *               ORBX_PD_OK iff R <= X <= width - 1 - R and R <= Y <= height - 1 - R, otherwise ORBX_PD_BORDER.  A slot
 *               that is not live or not usable is ORBX_PD_NONE
 *   D image     an OK slot is described on the image a level-0 keypoint of orbx_detect_and_compute is described on
 *               under the context's parameters: blurred iff blur_levels == 2, with the context's blur kind
 *   E values    for an OK slot, angle and the 32 descriptor bytes are the orientation (patch_size from the context)
 *               and the rotated BRIEF at (X, Y) on that image; rule C keeps every one of the 256 tests inside the
 *               image.  Every other slot has angle 0 and descriptor 0; n_ok[f] counts the OK slots.  Whole arrays
 *               compare equal
 *   F sets      only ORBX_PD_OK slots take part in a re-association, on both sides
 *   G 2-NN      for every query the best and the second-best train slot by Hamming distance; ties keep the lower
 *               train slot
 *   H accept    a second neighbour exists, (double)(float)d1 < ratio * (double)(float)d2 (the matcher's test,
 *               src/feature_tracking.cpp:213-217) and d1 <= max_distance
 *   I unique    (unique == 1) of several accepted queries with the same train slot the one with the smallest d1 keeps
 *               it, on a tie the lowest query slot; the others are rejected
 *   J out       origin[w][q] is the train slot or -1, dist[w][q] is d1 or -1, count[w] the accepted queries
 * Every device entry is asynchronous on the context's stream, or on `stream` (a hipStream_t) when that is not NULL; a
 * call waits on the device for the good-features, top-up and windows-tracker blocks it may read when they were written
 * on another stream, and orbx_landmarks_carry_device waits for the re-association's.  On any error nothing is launched
 * or written, the previous results stay fetchable and the context usable.  A call reads the caller's frames, points
 * and descriptors while it runs: a producer that replaces them on ANOTHER stream (the next good-features batch, whose
 * view the points are) has to be ordered behind it by the caller.
 * Not here: levels other than 0 (and with them a scale change between the two views), a position gate, refreshing a
 * landmark's descriptor across generations, a Harris response or octave per described point; no stream entry calls
 * the re-association. */
#ifndef ORBX_RELOC_H
#define ORBX_RELOC_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ORBX_PD_NONE = 0,   /* not live, or not usable (rule A) */
  ORBX_PD_BORDER = 1, /* usable, but closer than R to a border (rule C) */
  ORBX_PD_OK = 2      /* described */
} orbx_pd_state;

#define ORBX_PD_BANKS 2
/* The level-0 frames of a call (one byte per pixel, rows padded to a multiple of 4 bytes) live in a workspace of the
 * entry's own, allocated on demand and freed by orbx_destroy; above this many bytes the frames run in slices, with
 * identical results. */
#define ORBX_PD_WORKSPACE_DEFAULT ((size_t)512 << 20)

/* Rules A to E for n frames on the device -- d_frames, n, width, height, row_stride, frame_stride and stream as
 * orbx_good_features_batch_device takes them -- at a strided point source, as orbx_good_features_topup_device takes
 * its seeds: slot s of frame f is the two floats at d_xy + f * xy_frame_stride + s * point_stride (strides in floats),
 * d_seen (NULL: none) is int32 [n][slot_capacity] with seen_min, d_counts (NULL: none) int32 [n].  The LK windows view
 * (point_stride = 2 * window_len), the top-up view and the good-features view are valid sources.  Where the reference
 * runs ORB on the whole frame (src/feature_tracking.cpp:68-71) this describes the points the caller holds.  bank:
 * which of the context's ORBX_PD_BANKS result blocks is replaced; the other one and every other block stay as they
 * are.  ORBX_ERR_INVALID_ARG: the cases of orbx_good_features_batch_device, d_xy NULL, slot_capacity < 1, a bank
 * outside [0, ORBX_PD_BANKS), d_xy / d_seen / d_counts not 4-byte aligned, point_stride < 2 or xy_frame_stride <
 * point_stride * (slot_capacity - 1) + 2; ORBX_ERR_UNSUPPORTED: patch_size / 2 above 20, or more slots in the batch
 * than 32-bit offsets hold. */
int orbx_describe_points_device(orbx_ctx* ctx, const void* d_frames, int n, int width, int height, int row_stride,
                                size_t frame_stride, const float* d_xy, size_t point_stride, size_t xy_frame_stride,
                                const int32_t* d_seen, int seen_min, const int32_t* d_counts, int slot_capacity,
                                int bank, void* stream);
/* The workspace bound of orbx_describe_points_device in bytes (0: ORBX_PD_WORKSPACE_DEFAULT); at least one frame
 * always runs.  Waits for the entry's work and releases the workspace.  src/feature_tracking.cpp:68-71 */
int orbx_describe_points_workspace_limit(orbx_ctx* ctx, size_t bytes);
/* Device-side view of a bank, valid until the next call naming that bank.  Slots that are not ORBX_PD_OK hold
 * angle 0 and 32 zero bytes.  src/feature_tracking.cpp:68-71 */
typedef struct {
  const orbx_descriptor* desc; /* [n][slot_capacity] */
  const float* angle;          /* [n][slot_capacity], radians */
  const int32_t* state;        /* [n][slot_capacity]: an orbx_pd_state */
  const int32_t* n_ok;         /* [n] */
  int32_t slot_capacity, n;
} orbx_point_descriptors_view;
/* Fills the view; ORBX_ERR_INVALID_ARG for a bank outside [0, ORBX_PD_BANKS) or one that has not been written.
 * src/feature_tracking.cpp:68-71 */
int orbx_point_descriptors_results_device(orbx_ctx* ctx, int bank, orbx_point_descriptors_view* view);
/* Waits for the entry's work and copies frames [first, first + n) of a bank: desc (n x slot_capacity), angle, state
 * (n x slot_capacity each), n_ok (n); each may be NULL.  src/feature_tracking.cpp:68-71 */
int orbx_point_descriptors_fetch(orbx_ctx* ctx, int bank, int first, int n, orbx_descriptor* desc, float* angle,
                                 int32_t* state, int32_t* n_ok);
/* Rules A to E for ONE host image and n_points host points (x, y pairs), synchronous: angle, desc and state (n_points
 * each; each may be NULL).  It runs as a batch of one frame in bank 0 and replaces that bank.  n_points == 0 is a
 * no-op.  ORBX_ERR_INVALID_ARG: a bad image (as orbx_good_features_to_track), n_points < 0, points_xy NULL with
 * n_points > 0.  src/feature_tracking.cpp:68-71 */
int orbx_describe_points(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                         const float* points_xy, int n_points, float* angle, orbx_descriptor* desc, int32_t* state);

/* Rules F to J for n_windows pairs of described sets given by raw device pointers, so that any block can feed it:
 * query desc / state [n_windows][q_capacity], train desc / state [n_windows][t_capacity] (state: an orbx_pd_state per
 * slot), e.g. two banks' views.  Where the reference matches two ORB sets with a ratio test
 * (src/feature_tracking.cpp:203-219).  The result is a block of its own; every other block stays as it is.
 * ORBX_ERR_INVALID_ARG: a NULL array, one not aligned as its type (desc: 16 bytes), n_windows < 1, a capacity < 1, a
 * ratio that is not finite or negative, max_distance outside [0, 256], unique outside {0, 1}; ORBX_ERR_UNSUPPORTED:
 * n_windows above 65535, a capacity above 2^22, or more slots in the batch than 32-bit offsets hold. */
int orbx_reassociate_device(orbx_ctx* ctx, const orbx_descriptor* d_query_desc, const int32_t* d_query_state,
                            int q_capacity, const orbx_descriptor* d_train_desc, const int32_t* d_train_state,
                            int t_capacity, int n_windows, double ratio, int max_distance, int unique, void* stream);
/* Device-side view of the last re-association, valid until the next one.  origin has the shape
 * orbx_landmarks_carry_device takes as d_origin (slot_capacity = q_capacity).  src/feature_tracking.cpp:203-219 */
typedef struct {
  const int32_t* origin; /* [n_windows][q_capacity]: the train slot, or -1 */
  const int32_t* dist;   /* [n_windows][q_capacity]: the Hamming distance to it, or -1 */
  const int32_t* count;  /* [n_windows] */
  int32_t q_capacity, t_capacity, n_windows;
} orbx_reassociate_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before the first re-association.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate_results_device(orbx_ctx* ctx, orbx_reassociate_view* view);
/* Waits for the last re-association and copies windows [first, first + n): origin, dist (n x q_capacity each) and
 * count (n); each may be NULL.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate_fetch(orbx_ctx* ctx, int first, int n, int32_t* origin, int32_t* dist, int32_t* count);
/* Rules F to J for ONE window on HOST arrays, synchronous: outputs origin, dist (nq each) and count (one), each may
 * be NULL.  It runs as a re-association of one window and replaces that block.  nq == 0 writes count = 0 and launches
 * nothing.  ORBX_ERR_INVALID_ARG: nq < 0, nt < 0, a NULL input with a positive size, and the parameter cases of
 * orbx_reassociate_device.  src/feature_tracking.cpp:203-219 */
int orbx_reassociate(orbx_ctx* ctx, const orbx_descriptor* query_desc, const int32_t* query_state, int nq,
                     const orbx_descriptor* train_desc, const int32_t* train_state, int nt, double ratio,
                     int max_distance, int unique, int32_t* origin, int32_t* dist, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_RELOC_H */
