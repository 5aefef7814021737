// orbx_internal.h -- shared between the HIP kernels (orbx_*.hip) and the
// C-ABI host layer (orbx_api*.cpp, which share orbx_host.h among themselves).  Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx.h"

#include "orbx_plan.h"  // levels, plans, tile tables and their constants (host arithmetic, no HIP)

// pixel x of bit `b` of mask word `xw` of a row
__host__ __device__ inline int orbx_mask_x(const OrbxLevel& L, int xw, int b) {
  return L.mask_strip_px ? (xw >> 2) * L.mask_strip_px + (xw & 3) * 64 + b : xw * 64 + b;
}

// FAST early-exit state per frame (u64 words): tile-row statistics [level][band], then one
// "dead from band" word per level
#define ORBX_FAST_STAT_WORDS (ORBX_MAX_LEVELS * ORBX_MAX_BANDS + ORBX_MAX_LEVELS)
struct OrbxFastParams {
  int32_t threshold, n, nms_radius;
};

// ---- pyramidal Lucas-Kanade tracking (orbx_lk.hip) ---------------------------
#define ORBX_LK_MAX_LEVELS 8
struct OrbxLkLevel {
  const uint8_t* img;    // w x h, row pitch `pitch`
  const int16_t* deriv;  // Scharr (dx, dy) pairs, w x h tight; NULL in the `next` pyramid
  int32_t w, h, pitch, pad;
};
struct OrbxLkPyr {
  OrbxLkLevel L[ORBX_LK_MAX_LEVELS];
  int32_t top;  // highest level present
  int32_t pad;
};
hipError_t orbx_launch_lk_pyrdown(hipStream_t s, const uint8_t* d_src, int sw, int sh, int spitch, uint8_t* d_dst,
                                  int dw, int dh, int dpitch);
hipError_t orbx_launch_lk_scharr(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch, int16_t* d_deriv);
hipError_t orbx_launch_lk_track(hipStream_t s, const OrbxLkPyr& prev, const OrbxLkPyr& next, int n,
                                const float* d_prev_pts, float* d_next_pts, uint8_t* d_status, float* d_err, int win,
                                int max_iters, double eps2);
// The pyramids of the frames of one slice (k_lk_track_windows).  L describes frame `first`:
// level 0 is read IN PLACE from the caller's frames (L[0].img = frame 0 of the batch, frames frame_stride bytes
// apart), the levels above and every derivative map live in the workspace, img_stride bytes / der_stride int16
// apart from frame to frame.
struct OrbxLkFrames {
  OrbxLkLevel L[ORBX_LK_MAX_LEVELS];
  size_t frame_stride, img_stride, der_stride;
  int32_t top, first;
};
// the same kernels with the frame in blockIdx.z (frames <= 65535): one launch per level for a slice of frames
hipError_t orbx_launch_lk_pyrdown_frames(hipStream_t s, int frames, const uint8_t* d_src, int sw, int sh, int spitch,
                                         size_t src_frame_stride, uint8_t* d_dst, int dw, int dh, int dpitch,
                                         size_t dst_frame_stride);
hipError_t orbx_launch_lk_scharr_frames(hipStream_t s, int frames, const uint8_t* d_img, int w, int h, int pitch,
                                        size_t img_frame_stride, int16_t* d_deriv, size_t deriv_frame_bytes);
// grid (ceil(slot_capacity / 4), n_windows): n_windows <= 65535.  d_counts may be NULL (every slot is a point)
hipError_t orbx_launch_lk_track_windows(hipStream_t s, const OrbxLkFrames& frames, const int32_t* d_window_first,
                                        int n_windows, int window_len, const float* d_points, const int32_t* d_counts,
                                        int slot_capacity, float* d_tracks, int32_t* d_seen, float* d_err, int win,
                                        int max_iters, double eps2);
// the same with the forward-backward check (k_lk_track_windows_fb): thr2 = the squared
// threshold in binary64, >= 0 (+inf included); d_fb_d2 [n_windows][slot_capacity][window_len - 1], d_lost
// [n_windows][slot_capacity]
hipError_t orbx_launch_lk_track_windows_fb(hipStream_t s, const OrbxLkFrames& frames, const int32_t* d_window_first,
                                           int n_windows, int window_len, const float* d_points,
                                           const int32_t* d_counts, int slot_capacity, float* d_tracks, int32_t* d_seen,
                                           float* d_err, float* d_fb_d2, int32_t* d_lost, int win, int max_iters,
                                           double eps2, double thr2);

// ---- launchers (orbx_kernels.hip) ------------------------------------------
// All take the stream explicitly and never synchronise or allocate.
// d_tiles: tiles of ONE frame for 256 x 16 tiles
hipError_t orbx_launch_pyramid2(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int frame_bytes, int w0,
                                int h0, int n_frames, const uint8_t* d_in, int in_stride, size_t in_frame_stride,
                                const OrbxResizeTap* d_taps, uint8_t* d_pyr);
hipError_t orbx_launch_blur(hipStream_t s, const OrbxPlan& plan, const OrbxTileMap& tm, int n_frames,
                            const uint8_t* d_src, uint8_t* d_dst, int first_level, int kind);
// d_tiles: strip table of ONE frame (level, strip, first row, rows)
hipError_t orbx_launch_blur3(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int frame_bytes, int n_frames,
                             const uint8_t* d_src, uint8_t* d_dst, int first_level);
hipError_t orbx_launch_blur4(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int frame_bytes, int n_frames,
                             const uint8_t* d_src, uint8_t* d_dst, int first_level);
// d_tiles: strip table of ONE frame with the pyramid fields (u0 / u1 / u2 = xtab_off / ytab_off / win8)
hipError_t orbx_launch_pyrblur(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int frame_bytes, int w0, int h0,
                               int n_frames, const uint8_t* d_in, int in_stride, size_t in_frame_stride,
                               const OrbxResizeTap* d_taps, uint8_t* d_dst, int group = 0,
                               const unsigned long long* d_row_stat = nullptr, uint32_t* d_feedback = nullptr,
                               const OrbxTopLevels* top = nullptr, unsigned long long* d_zero_stat = nullptr);
// d_tiles: n_tiles OrbxTileDesc in band-major order (orbx_api.cpp: build_fast_tiles, tile height
// orbx_fast3_tile_h(fp.nms_radius)); d_scores: optional dense u16 score map of ONE frame (stage operator)
hipError_t orbx_launch_fast_nms(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int n_frames,
                                const uint8_t* d_pyr, int frame_bytes, int mask_words, OrbxFastParams fp,
                                unsigned long long* d_mask, uint16_t* d_scores,
                                unsigned long long* d_row_stat, int chunk_scale = 1);
// streaming FAST + NMS of the whole path: d_tiles = (strip, tile row) units of ONE frame in band-major order, masks in
// strip layout (OrbxLevel::mask_strip_px > 0)
hipError_t orbx_launch_fast4(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int n_frames, const uint8_t* d_pyr,
                             int frame_bytes, int mask_words, OrbxFastParams fp, unsigned long long* d_mask,
                             unsigned long long* d_row_stat);
hipError_t orbx_launch_compact(hipStream_t s, const OrbxPlan& plan, int n_frames,
                               const unsigned long long* d_mask, orbx_keypoint* d_cand, int32_t* d_cand_count,
                               int32_t* d_cand_total, int need_total);
hipError_t orbx_launch_harris_flat(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch,
                                   const orbx_keypoint* d_kps, int nkp, const float* d_gauss, int K, float kk,
                                   float* d_resp);
// fused compaction + Harris + selection, one workgroup per (level, frame)
hipError_t orbx_launch_level_select(hipStream_t s, const OrbxPlan& plan, int n_frames, int mode,
                                    const unsigned long long* d_mask, const uint8_t* d_pyr, const float* d_gauss,
                                    int window, float k, orbx_keypoint* d_sel_lkp, float* d_sel_resp,
                                    int32_t* d_sel_count, uint32_t* d_need = nullptr);
// fused kernel or the three spread kernels, chosen by shape (force: 0 fused, 1 spread, -1 auto);
// d_cand / d_cresp: cand_total slots per frame, d_ncand: nlevels per frame (spread path only)
hipError_t orbx_launch_level_select_auto(hipStream_t s, const OrbxPlan& plan, int n_frames, int mode, int force,
                                         const unsigned long long* d_mask, const uint8_t* d_pyr,
                                         const float* d_gauss, int window, float k, uint32_t* d_cand,
                                         int32_t* d_ncand, float* d_cresp, orbx_keypoint* d_sel_lkp,
                                         float* d_sel_resp, int32_t* d_sel_count, uint32_t* d_need = nullptr);
// device-visible addresses of the compact sections of a result block's pinned host mirror (all null: not wanted)
struct OrbxHostRecord {
  int32_t* counts;
  uint32_t* kp16;
  float* angle;
  orbx_descriptor* desc;
};
hipError_t orbx_launch_describe(hipStream_t s, const OrbxPlan& plan, int n_frames, const uint8_t* d_pyr,
                                int patch_size, const int32_t* d_sel_count, const orbx_keypoint* d_sel_lkp,
                                const float* d_sel_resp, int32_t* d_out_count, orbx_keypoint* d_out_lkp,
                                float* d_out_resp, int32_t* d_out_level, orbx_keypoint* d_out_kp, uint32_t* d_out_kp16,
                                float* d_out_angle, orbx_descriptor* d_out_desc, const uint32_t* d_feedback = nullptr,
                                uint32_t* h_feedback = nullptr, const OrbxHostRecord* host_record = nullptr);

// stage-level helpers on plain (single-image, arbitrary pitch) buffers
hipError_t orbx_launch_describe_flat(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch,
                                     const orbx_keypoint* d_kps, int nkp, int patch_size, int use_given_angles,
                                     int do_brief, float* d_angles, orbx_descriptor* d_desc);
hipError_t orbx_launch_nms_f32(hipStream_t s, const float* d_scores, int w, int h, int radius, float threshold,
                               unsigned long long* d_mask, int mask_wpr);
hipError_t orbx_launch_conv2d(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch, const float* d_kernel,
                              int K, int reflect_pad, uint8_t* d_dst, int dst_pitch);
hipError_t orbx_launch_select_flat(hipStream_t s, const float* d_resp, int n, int keep, int32_t* d_idx);

// 256-bit Hamming 2-NN + ratio test over `npairs` (query set, train set) pairs
hipError_t orbx_launch_knn2(hipStream_t s, int npairs, int max_nq, const orbx_descriptor* d_q, const int32_t* d_qcount,
                            size_t qstride, const orbx_descriptor* d_t, const int32_t* d_tcount, size_t tstride,
                            double ratio, int32_t* d_idx, int32_t* d_dist, int32_t* d_match, size_t ostride);

// relative pose (orbx_pose.hip): one normalised correspondence, one pair's result
struct OrbxPosePt {
  double x1, y1, x2, y2;
};
struct OrbxPoseOut {
  double E[9], R[9], t[3];
  int32_t inliers, good, iters, pad;
};
hipError_t orbx_launch_pose_prep_batch(hipStream_t s, int npairs, int cap, const int32_t* d_counts,
                                       const orbx_keypoint* d_kp, const int32_t* d_match, const double* K,
                                       OrbxPosePt* d_pts, int32_t* d_npts);
hipError_t orbx_launch_pose_prep_host(hipStream_t s, int n, const float* d_p1, const float* d_p2, const double* K,
                                      OrbxPosePt* d_pts, int32_t* d_npts);
hipError_t orbx_launch_pose_ransac(hipStream_t s, int npairs, int cap, const OrbxPosePt* d_pts, const int32_t* d_npts,
                                   const double* K, double prob, double threshold, int max_iters, uint64_t seed,
                                   OrbxPoseOut* d_out, uint8_t* d_mask);

// triangulation and relative scale (orbx_scale.hip): one pair's result
struct OrbxScaleOut {
  double scale;
  int32_t triplets, ratios_used;
};
// dynamic LDS a scale kernel may ask for: a workgroup's 160 KB on gfx950 less 256 bytes for the kernels' static
// variables; k_scale_join needs 16 bytes per result slot (at most 10 224), k_scale_aligned 8 per point (20 448)
#define ORBX_SCALE_LDS_MAX (160 * 1024 - 256)
// d_xyz / d_valid / d_mq / d_mt: one row of `cap` per pair, in the compact query order of orbx_batch_match_fetch
// (the point, its valid byte, the match's query and train index); d_npts: matches per pair
hipError_t orbx_launch_triangulate_batch(hipStream_t s, int npairs, int cap, const int32_t* d_counts,
                                         const orbx_keypoint* d_kp, const int32_t* d_match, const OrbxPoseOut* d_pose,
                                         const double* K, float* d_xyz, uint8_t* d_valid, int32_t* d_mq, int32_t* d_mt,
                                         int32_t* d_npts);
hipError_t orbx_launch_triangulate_host(hipStream_t s, int n, const float* d_p1, const float* d_p2, const double* K,
                                        const double* R, const double* t, float* d_xyz, uint8_t* d_valid);
// chain: consecutive pairs per chain (>= 1); the first pair of every chain has no predecessor
hipError_t orbx_launch_scale_join(hipStream_t s, int npairs, int chain, int cap, const int32_t* d_npts, const int32_t* d_mq,
                                  const int32_t* d_mt, const float* d_xyz, const uint8_t* d_valid,
                                  const OrbxPoseOut* d_pose, OrbxScaleOut* d_out);
// a NULL valid array: every point is valid
hipError_t orbx_launch_scale_aligned(hipStream_t s, int n_prev, int n_cur, const float* d_prev,
                                     const uint8_t* d_prev_valid, const float* d_cur, const uint8_t* d_cur_valid,
                                     OrbxScaleOut* d_out);

// ---- bundle adjustment (orbx_ba.hip): one workgroup per window, each owning a workspace ----------------------
// workspace doubles per landmark (accepted and candidate point, V, gradient, Jacobi scale, inverse block, scaled
// gradient, damping) and per observation (the 6x3 coupling block W)
#define ORBX_BA_WS_POINT 30
#define ORBX_BA_WS_OBS 18
// landmarks of one window: bounded so that 32-bit indices into a workspace row never overflow and a window of
// 5 poses x 4096 landmarks fits with room to spare
#define ORBX_BA_MAX_POINTS 65536
// workgroups per launch: each solves windows group, group + groups, ... (bounds the workspace); fewer when their
// workspaces together would exceed the budget
#define ORBX_BA_MAX_GROUPS 512
#define ORBX_BA_WS_BUDGET ((size_t)2 << 30)
// d_rows: per window, (landmarks + 1) offsets into the window's observations, window w's first at
// d_pt_off[w] + w; d_out: one BaSummary (= orbx_ba_summary) per window; K4 = fx, fy, cx, cy
hipError_t orbx_launch_ba(hipStream_t s, int n_windows, int groups, int max_iters, const double* K4, double delta,
                          const int32_t* d_pose_off, const int32_t* d_pt_off, const int32_t* d_obs_off,
                          double* d_poses, double* d_points, const int32_t* d_rows, const uint8_t* d_obs_pose,
                          const double* d_obs_xy, int cap, int ocap, double* d_ws_pt, double* d_ws_obs,
                          unsigned long long* d_ws_slot, void* d_out);
// the same solve with landmark priors: d_prior holds anchor (3) and weight (1) of every landmark
// in the batch's point order, landmark j of window w at 4 * (d_pt_off[w] + j); start: an orbx_prior_start
hipError_t orbx_launch_ba_prior(hipStream_t s, int n_windows, int groups, int max_iters, const double* K4, double delta,
                                const int32_t* d_pose_off, const int32_t* d_pt_off, const int32_t* d_obs_off,
                                double* d_poses, double* d_points, const int32_t* d_rows, const uint8_t* d_obs_pose,
                                const double* d_obs_xy, int cap, int ocap, double* d_ws_pt, double* d_ws_obs,
                                unsigned long long* d_ws_slot, void* d_out, const double* d_prior, int start);

// ---- landmarks of tracked windows (orbx_landmarks.hip) ---------------------------------------
// The block k_lm_fill writes is the block orbx_launch_ba reads: status [n], three offset arrays [n + 1], points3
// (3 doubles per kept landmark), rows (window w's landmarks + 1 offsets at pt_off[w] + w), opose / oxy per
// observation, and the slot each kept landmark came from.  Sized for every slot kept: n * cap points, n * cap + n
// rows, n * cap * window_len observations.
#define ORBX_LM_THREADS 256
struct OrbxLmBlock {
  int32_t *status, *pose_off, *pt_off, *obs_off;
  double* points3;
  int32_t* rows;
  uint8_t* opose;
  double* oxy;
  int32_t* slot_of_point;
};
// workgroups of k_lm_triangulate per window = rows of its table of partial counts
inline int orbx_lm_blocks(int cap) { return (cap + ORBX_LM_THREADS - 1) / ORBX_LM_THREADS; }
// K9: row-major 3x3 (host); d_poses: 6 * window_len doubles per window; d_tracks / d_seen: the layout of
// orbx_lk_windows_view; d_cand: 3 rows of n * cap doubles; d_keep: n * cap bytes; d_partial: 2 * n * blocks; d_gate: n;
// d_pose_status: NULL, or the status per window of poses chained on the device (orbx_launch_window_poses): a window
// that is not 0 there is ORBX_LM_BAD_POSE
hipError_t orbx_launch_landmarks(hipStream_t s, const double* K9, const double* d_poses, const float* d_tracks,
                                 const int32_t* d_seen, int n_windows, int cap, int window_len, double* d_cand,
                                 uint8_t* d_keep, int32_t* d_partial, int32_t* d_gate, const OrbxLmBlock& out,
                                 const int32_t* d_pose_status = nullptr);
// the build from every view of a track: tri_mode and max_reproj_px as include/orbx_lm.h has
// them; d_table: 16 doubles per (window, view); d_reason / d_reproj_px: n * cap each; the rest as above
hipError_t orbx_launch_landmarks_views(hipStream_t s, const double* K9, const double* d_poses, const float* d_tracks,
                                       const int32_t* d_seen, int n_windows, int cap, int window_len, int tri_mode,
                                       double max_reproj_px, double* d_table, uint8_t* d_reason, float* d_reproj_px,
                                       double* d_cand, uint8_t* d_keep, int32_t* d_partial, int32_t* d_gate,
                                       const OrbxLmBlock& out, const int32_t* d_pose_status = nullptr);

// ---- window poses and the write-back gate (orbx_wposes.hip) ---------------------------------
// d_pose / d_scale: the tracks-pose block's rows, window w's pairs at w * (window_len - 1); d_T0: 16 doubles and
// d_scale0: one per window; d_poses6 / d_poses4x4: 6 / 16 doubles per frame, window-major; d_status: one per window
hipError_t orbx_launch_window_poses(hipStream_t s, int n_windows, int window_len, const OrbxPoseOut* d_pose,
                                    const OrbxScaleOut* d_scale, const double* d_T0, const double* d_scale0,
                                    double* d_poses6, double* d_poses4x4, int32_t* d_status);
// d_solved6 / d_built6: the blocks after the solve and as built; d_summaries: one orbx_ba_summary per window;
// d_poses4x4: 16 doubles and d_updated: one byte per (window, pose)
hipError_t orbx_launch_ba_write_back(hipStream_t s, int n_windows, int window_len, const double* d_solved6,
                                     const double* d_built6, const void* d_summaries, double max_rot,
                                     double max_trans, double* d_poses4x4, uint8_t* d_updated);

// ---- perspective-n-point with RANSAC (orbx_pnp.hip) -----------------------------------------
// one correspondence of a problem: the world point and its pixel
struct OrbxPnpCorr {
  double X[3], x, y;
};
struct OrbxPnpRecord {  // = orbx_pnp_record
  double pose6[6];
  int32_t inliers, iters, n_corr, status;
  double rms_px;
};
// what a batch reads: sections of the landmarks block and the poses it was built from.  status == NULL: ONE problem
// whose n_pre correspondences are in d_corr already (the host-array entry), with `seed` as its own seed
struct OrbxPnpIn {
  const int32_t *status, *pt_off, *obs_off, *rows;
  const double *points3, *oxy, *built6;
};
// One workgroup per problem (window w, frame k >= 2), problem w * (window_len - 2) + k - 2.  d_corr / d_cidx / d_mask:
// one row of `cap` per problem; d_rec: one record per problem; d_seeded6: 6 doubles per (window, frame).  The seed of
// problem (w, k) is pnp_problem_seed(seed, k).
hipError_t orbx_launch_pnp(hipStream_t s, int n_windows, int window_len, int cap, const OrbxPnpIn& in, int n_pre,
                           const double* K4, double prob, double threshold_px, int max_iters, uint64_t seed,
                           int refine_iters, int min_inliers, OrbxPnpCorr* d_corr, int32_t* d_cidx,
                           OrbxPnpRecord* d_rec, double* d_seeded6, uint8_t* d_mask,
                           const int32_t* d_ncorr = nullptr);
// d_ncorr != NULL (rank 18; `in` empty, d_seeded6 NULL): one workgroup per (window, frame k >= 0), problem
// w * window_len + k, every row of d_corr / d_cidx gathered already by orbx_launch_carry_gather; d_ncorr: the
// problem's count, or -1 for ORBX_PNP_SKIPPED; the mask is indexed by d_cidx (the slot)

// ---- landmarks carried into the next window (orbx_carry.hip) --------------------------------
enum { CARRY_OK = 0, CARRY_LOST = 1 };
// the old block a carry reads: status [n], pt_off [n + 1], the ascending slot_of_point and the coordinates (3 doubles)
// of every landmark, and the old windows' slot capacity
struct OrbxCarryIn {
  const int32_t *status, *pt_off, *slot;
  const double* src;
  int old_cap;
};
// d_origin / d_point: n_windows * cap; d_xyz: 3 doubles per slot; d_count: one per window
hipError_t orbx_launch_carry_join(hipStream_t s, const OrbxCarryIn& in, const int32_t* d_origin, int n_windows, int cap,
                                  double* d_xyz, int32_t* d_point, int32_t* d_count);
// d_corr / d_cidx: one row of `cap` per problem (w, k), problem w * window_len + k; d_ncorr: one per problem
hipError_t orbx_launch_carry_gather(hipStream_t s, const double* d_xyz, const int32_t* d_point, const int32_t* d_count,
                                    const float* d_tracks, const int32_t* d_seen, int n_windows, int cap, int window_len,
                                    OrbxPnpCorr* d_corr, int32_t* d_cidx, int32_t* d_ncorr);
// d_rec: window_len records per window; d_poses6: 6 doubles per (window, frame); d_wstatus: one per window
hipError_t orbx_launch_carry_fill(hipStream_t s, const OrbxPnpRecord* d_rec, int n_windows, int window_len,
                                  double* d_poses6, int32_t* d_wstatus);

// ---- landmark priors of a carried window (orbx_prior.hip; DESIGN.md §9 rank 20, rule P6) ---------------------------
// d_status / d_pt_off / d_slot_of_point: the landmarks block's; d_carry_xyz / d_carry_point: the carry block's, of the
// same n_windows and cap; d_prior: 4 doubles per landmark in the block's point order; d_count: one per window
hipError_t orbx_launch_prior_gather(hipStream_t s, const int32_t* d_status, const int32_t* d_pt_off,
                                    const int32_t* d_slot_of_point, const double* d_carry_xyz,
                                    const int32_t* d_carry_point, int n_windows, int cap, double weight,
                                    double* d_prior, int32_t* d_count);

// ---- descriptors at caller-held points and the re-association (orbx_reloc.hip) --------------
enum { PD_NONE = 0, PD_BORDER = 1, PD_OK = 2 };  // = orbx_pd_state
#define PD_R_MIN 20  // rule C: the BRIEF pattern's reach (18) plus the 5x5 box (2)
// how k_pd_level0 makes the level-0 image: an orbx_blur_kind, or the plain copy
#define PD_LEVEL0_COPY 2
// d_level0: n images of pitch x h bytes (pitch a multiple of 4, >= w), img_stride (a multiple of 4) apart
hipError_t orbx_launch_pd_level0(hipStream_t s, const uint8_t* d_frames, int n, int w, int h, int row_stride,
                                 size_t frame_stride, int kind, uint8_t* d_level0, int pitch, size_t img_stride);
// n <= 65535 frames.  d_xy / d_seen / d_counts: the point source of frame 0 of the n (d_seen, d_counts may be NULL);
// d_state / d_angle / d_desc / d_list: one row of `cap` per frame; d_n_ok: one per frame.  d_list is scratch
hipError_t orbx_launch_pd_describe(hipStream_t s, const uint8_t* d_level0, int n, int w, int h, int pitch,
                                   size_t img_stride, const float* d_xy, size_t point_stride, size_t xy_frame_stride,
                                   const int32_t* d_seen, int seen_min, const int32_t* d_counts, int cap, int patch_size,
                                   int32_t* d_state, float* d_angle, orbx_descriptor* d_desc, int32_t* d_n_ok,
                                   int32_t* d_list);
// n_windows <= 65535, qcap <= 2^22.  d_best: n_windows * tcap words of scratch (unique only); d_origin / d_dist:
// n_windows * qcap; d_count: one per window
hipError_t orbx_launch_reassociate(hipStream_t s, int n_windows, const orbx_descriptor* d_qdesc,
                                   const int32_t* d_qstate, int qcap, const orbx_descriptor* d_tdesc,
                                   const int32_t* d_tstate, int tcap, double ratio, int max_distance, int unique,
                                   uint32_t* d_best, int32_t* d_origin, int32_t* d_dist, int32_t* d_count);

// rules I-J alone, on origin / dist / best as a 2-NN kernel left them (the gated re-association of rank 21 ends with it)
hipError_t orbx_launch_ra_unique(hipStream_t s, int n_windows, int qcap, int tcap, int unique, const uint32_t* d_best,
                                 int32_t* d_origin, int32_t* d_dist, int32_t* d_count);

// ---- the search by projection (orbx_search.hip) ----------------------------------------------
// `in`: the old block as the carry reads it; d_pose6: one predicted pose per window, pose_stride doubles apart; K4 (host)
// = fx, fy, cx, cy; d_xy: 2 doubles per slot, d_depth / d_state: one per slot, d_count: one per window.  cap <= 65536
hipError_t orbx_launch_sp_project(hipStream_t s, const OrbxCarryIn& in, int n_windows, int cap, const double* d_pose6,
                                  size_t pose_stride, const double* K4, int width, int height, double margin_px,
                                  double* d_xy, double* d_depth, int32_t* d_state, int32_t* d_count);
// the most cells of a window's grid: its counts, then its starts, are one LDS table of a workgroup
#define ORBX_SG_CELLS_MAX 4096
// a window's grid: cell (cx, cy) = clamped floor((x - x0) * inv), floor((y - y0) * inv), nx * ny <= ORBX_SG_CELLS_MAX
struct OrbxSgGrid {
  double x0, y0, inv;
  int32_t nx, ny;
};
// n_windows <= 65535, capacities <= 2^22.  Scratch: d_grids: one per window; d_starts: ORBX_SG_CELLS_MAX + 1 per window;
// d_sslot / d_sxy (2 doubles) / d_sdesc: one per train slot, the window's positioned OK train slots in cell order;
// d_best: n_windows * tcap words (unique only).  d_origin / d_dist / d_candidates: n_windows * qcap; d_count: one per
// window.  d_tpstate may be NULL
hipError_t orbx_launch_reassociate_gated(hipStream_t s, int n_windows, const orbx_descriptor* d_qdesc,
                                         const int32_t* d_qstate, const float* d_qxy, size_t point_stride,
                                         size_t xy_frame_stride, int qcap, const orbx_descriptor* d_tdesc,
                                         const int32_t* d_tstate, const double* d_txy, const int32_t* d_tpstate,
                                         int tcap, double radius_px, double ratio, int max_distance, int accept_lone,
                                         int unique, OrbxSgGrid* d_grids, int32_t* d_starts, int32_t* d_sslot,
                                         double* d_sxy, orbx_descriptor* d_sdesc, uint32_t* d_best, int32_t* d_origin,
                                         int32_t* d_dist, int32_t* d_candidates, int32_t* d_count);

// ---- overlapping windows joined into one trajectory (orbx_stitch.hip) ------------------------
// Window w of window_len frames starts at stream frame w * stride, 1 <= stride <= window_len - 1.
// d_scale: the tracks-pose block's scale rows; d_scale0: one double per window (the chain's input section)
hipError_t orbx_launch_st_scale0(hipStream_t s, int n_windows, int window_len, int stride, double scale0_first,
                                 const OrbxScaleOut* d_scale, double* d_scale0);
// d_poses4x4: 16 doubles per (window, frame); d_T_start: 16 doubles; d_links: 14 doubles and d_broken: one int32 per
// window (scratch); d_trajectory4x4 / d_owner: per stream frame; d_anchors4x4 / d_lambda / d_status: per window
hipError_t orbx_launch_stitch(hipStream_t s, int n_windows, int window_len, int stride, const double* d_poses4x4,
                              const double* d_T_start, int align_scale, double* d_links, int32_t* d_broken,
                              double* d_trajectory4x4, int32_t* d_owner, double* d_anchors4x4, double* d_lambda,
                              int32_t* d_status);

// ---- pose and scale of tracked frame pairs (orbx_tracks.hip) --------------------------------
// Window w of window_len frames owns window_len - 1 pairs, pair p = w * (window_len - 1) + k is frames k, k + 1.
// Every per-position array has one row of `cap` = slot_capacity per pair.
// d_tracks / d_seen: the layout of orbx_lk_windows_view.  Writes, per pair, the compacted list of the slots with
// seen >= k + 2 in ascending slot order: d_pts (what k_pose_ransac reads), d_slot_of, d_npts; and zeroes
// d_slot_of, d_mask, d_xyz and d_valid past the list.
hipError_t orbx_launch_tracks_prep(hipStream_t s, int n_windows, int cap, int window_len, const float* d_tracks,
                                   const int32_t* d_seen, const double* K, OrbxPosePt* d_pts, int32_t* d_npts,
                                   int32_t* d_slot_of, uint8_t* d_mask, float* d_xyz, uint8_t* d_valid);
// rank 6 rule 1 over the compacted lists, with the pair's own R, t
hipError_t orbx_launch_tracks_triangulate(hipStream_t s, int n_windows, int cap, int window_len, const float* d_tracks,
                                          const int32_t* d_npts, const int32_t* d_slot_of, const OrbxPoseOut* d_pose,
                                          const double* K, float* d_xyz, uint8_t* d_valid);

// ---- Shi-Tomasi corners (orbx_gftt.hip): n frames per launch, every array per frame ---------
// d_map: w * h floats; d_max: the largest response as a bit pattern (zeroed by the caller); d_keys: `pool` =
// (w - 2)(h - 2) keys; d_ncand: candidates (zeroed by the caller); d_grid: grid_stride >= gw * gh * slots words, all
// 0xff (min_distance >= 1 only); cap: result slots
hipError_t orbx_launch_gftt_response(hipStream_t s, const uint8_t* d_frames, int n, int w, int h, int row_stride,
                                     size_t frame_stride, float* d_map, uint32_t* d_max);
hipError_t orbx_launch_gftt_candidates(hipStream_t s, const float* d_map, int n, int w, int h, const uint32_t* d_max,
                                       double quality, unsigned long long* d_keys, size_t pool, int32_t* d_ncand);
hipError_t orbx_launch_gftt_select(hipStream_t s, int n, int w, unsigned long long* d_keys, size_t pool,
                                   const int32_t* d_ncand, double min_distance, int cell, int gw, int gh, int slots,
                                   uint32_t* d_grid, size_t grid_stride, int cap, int32_t* d_counts,
                                   float* d_corners);
// rank 12 (top-up): d_bits: ceil(w / 32) * h words per frame, a set bit blocks the pixel (zeroed by the caller before
// orbx_launch_gftt_block, which ORs the carried seeds' neighbourhoods in; orbx_launch_gftt_mask_bits writes every
// word of ONE frame); d_mmax: the largest unblocked response (zeroed by the caller); d_seed_xy may be NULL (no seeds);
// max_seeds: the most seeds a frame can carry (sizes the blocking launch); slot_cap: result slots per frame
hipError_t orbx_launch_gftt_seeds(hipStream_t s, int n, const float* d_seed_xy, size_t point_stride,
                                  size_t frame_stride, const int32_t* d_seed_seen, int seen_min, int seed_cap, int w,
                                  int h, int slot_cap, int32_t* d_carried, float* d_points, int32_t* d_origin);
hipError_t orbx_launch_gftt_block(hipStream_t s, int n, const float* d_points, const int32_t* d_carried, int slot_cap,
                                  int max_seeds, int w, int h, double min_distance, uint32_t* d_bits);
hipError_t orbx_launch_gftt_mask_bits(hipStream_t s, const uint8_t* d_mask, int w, int h, int mask_stride,
                                      uint32_t* d_bits);
hipError_t orbx_launch_gftt_masked_max(hipStream_t s, const float* d_map, int n, int w, int h, const uint32_t* d_bits,
                                       uint32_t* d_mmax);
hipError_t orbx_launch_gftt_candidates_blocked(hipStream_t s, const float* d_map, int n, int w, int h,
                                               const uint32_t* d_mmax, double quality, unsigned long long* d_keys,
                                               size_t pool, int32_t* d_ncand, const uint32_t* d_bits);
hipError_t orbx_launch_gftt_select_topup(hipStream_t s, int n, int w, unsigned long long* d_keys, size_t pool,
                                         const int32_t* d_ncand, double min_distance, int cell, int gw, int gh,
                                         int slots, uint32_t* d_grid, size_t grid_stride, int slot_cap,
                                         const int32_t* d_carried, int32_t* d_counts, float* d_points);
