// orbx_landmarks.hip -- landmarks of many tracked windows, built on the device in the layout k_ba_lm reads
// (DESIGN.md §9, rank 10).
//
// Replaces buildLandmarksFromFirstTwoFramesAndTracks (src/with_bundle_adjustment.cpp:502-575) for n_windows windows
// per call: the tracks of orbx_lk_track_windows_device in, the CSR block of orbx_launch_ba out, no host round trip.
//   k_lm_triangulate  one lane per (window, slot): gate and projections per wave from uniform loads, the DLT and the
//                     depth check per lane; candidate point and keep flag into a slot-indexed scratch (SoA), the
//                     workgroup's kept landmarks and kept observations into a table of partial counts
//   k_lm_offsets      one workgroup: the partial counts of every window summed, the statuses, and the exclusive scan
//                     of both counts over the windows in chunks of the workgroup size
//   k_lm_fill         one workgroup per window: slots in chunks of the workgroup size, ballot / wave scan / LDS
//                     across the waves with a carried base, plain stores -- kept landmarks stay in slot order
// The build from every view of a track with its reprojection gate (rank 15) puts two kernels of its own in front of
// the same k_lm_offsets and k_lm_fill:
//   k_lm_views              one lane per (window, view): the pose prepared once, P_k and the depth row into a 16-double
//                           record of the window's table, the window's gate from the eight lanes of its views
//   k_lm_triangulate_views  k_lm_triangulate's grid and outputs; the window's table is read with uniform addresses,
//                           the normal matrix is summed view by view, the sweeps are tri_homogeneous's own, and the
//                           depth and reprojection pass reads the table again; reason and reproj_px per slot
// All arithmetic comes from orbx_lm_math.h, compiled with -ffp-contract=off, so every result equals the sequential
// restatement (tests/cpp/lm_sequential.cpp, tests/cpp/lm_views_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"
#include "orbx_wave.h"

namespace {

constexpr int LM_THREADS = ORBX_LM_THREADS;
static_assert(LM_THREADS == 256, "four waves: the cross-wave prefixes below are written out for four");

struct LmK9 {
  double k[9];
};

// exclusive prefix over the four waves of two per-wave totals (a: lanes' flags, b: lanes' observation counts), and
// the workgroup's totals; between two barriers
struct LmWaves {
  int a[4], b[4];
};
__device__ __forceinline__ void lm_cross_wave(LmWaves& S, int wave_a, int wave_b, int* pre_a, int* pre_b, int* tot_a,
                                              int* tot_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) S.a[wave] = wave_a, S.b[wave] = wave_b;
  __syncthreads();
  int pa = 0, pb = 0, ta = 0, tb = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i < wave) pa += S.a[i], pb += S.b[i];
    ta += S.a[i], tb += S.b[i];
  }
  *pre_a = pa, *pre_b = pb, *tot_a = ta, *tot_b = tb;
  __syncthreads();  // S may be rewritten
}

__global__ __launch_bounds__(LM_THREADS) void k_lm_triangulate(LmK9 K, const double* __restrict__ poses,
                                                               const float* __restrict__ tracks,
                                                               const int32_t* __restrict__ seen, int cap,
                                                               int window_len, int nblk, size_t total,
                                                               double* __restrict__ cand, uint8_t* __restrict__ keep,
                                                               int32_t* __restrict__ partial,
                                                               int32_t* __restrict__ gate,
                                                               const int32_t* __restrict__ pose_status) {
  __shared__ LmWaves S;
  const int tid = threadIdx.x;
  const int win = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int slot = blk * LM_THREADS + tid;
  const size_t idx = (size_t)win * cap + slot;
  // rules 1-2: the same for every lane of the window
  const double* pose = poses + 6 * (size_t)window_len * win;
  double P0[12], P1[12];
  int status = lm_window_prepare(K.k, pose, pose + 6, P0, P1);
  // poses chained on the device (rank 14): a window whose chain is not finite is a bad pose and owns no landmark
  if (pose_status && pose_status[win] != 0) status = LM_BAD_POSE;
  double X[3] = {0.0, 0.0, 0.0};
  bool kept = false;
  int obs = 0;
  if (status == LM_OK && slot < cap) {
    const int sn = lm_seen(seen[idx], window_len);
    if (sn >= 2) {
      const float* t = tracks + 2 * (size_t)window_len * idx;
      kept = lm_point(P0, P1, t[0], t[1], t[2], t[3], X);
      obs = kept ? sn : 0;
    }
  }
  if (slot < cap) {
#pragma unroll
    for (int k = 0; k < 3; k++) cand[k * total + idx] = X[k];
    keep[idx] = kept ? 1 : 0;
  }
  const int wave_kept = __popcll(__ballot(kept)), wave_obs = wave_sum(obs);
  int pa, pb, ta, tb;
  lm_cross_wave(S, wave_kept, wave_obs, &pa, &pb, &ta, &tb);
  if (tid == 0) {
    partial[2 * (size_t)blockIdx.x] = ta;
    partial[2 * (size_t)blockIdx.x + 1] = tb;
    if (blk == 0) gate[win] = status;
  }
}

static_assert(ORBX_BA_MAX_POSES == 8, "k_lm_views: the eight lanes of a window's views share a wave");

__global__ __launch_bounds__(LM_THREADS) void k_lm_views(LmK9 K, const double* __restrict__ poses, int n_windows,
                                                         int window_len, int n_prep,
                                                         const int32_t* __restrict__ pose_status,
                                                         double* __restrict__ table, int32_t* __restrict__ gate) {
  const int t = blockIdx.x * LM_THREADS + threadIdx.x;
  const int win = t >> 3, view = t & 7;
  const double* pose = poses + 6 * ((size_t)window_len * (win < n_windows ? win : 0));
  int ok = 1;
  if (win < n_windows && view < n_prep) {
    double rec[LM_VIEW_DOUBLES];
    ok = lm_view_prepare(K.k, pose + 6 * view, rec);
    double* out = table + LM_VIEW_DOUBLES * ((size_t)window_len * win + view);
#pragma unroll
    for (int i = 0; i < LM_VIEW_DOUBLES; i++) out[i] = rec[i];
  }
  // rule 1: every prepared pose has to be ok, then the baseline of poses 0 and 1
  const unsigned ok8 = (unsigned)(__ballot(ok != 0) >> (threadIdx.x & 56)) & 0xffu;
  if (win < n_windows && view == 0) {
    int status = ok8 != 0xffu ? LM_BAD_POSE : lm_baseline(pose + 3, pose + 9);
    if (pose_status && pose_status[win] != 0) status = LM_BAD_POSE;
    gate[win] = status;
  }
}

__global__ __launch_bounds__(LM_THREADS) void k_lm_triangulate_views(
    const double* __restrict__ table, const int32_t* __restrict__ gate, const float* __restrict__ tracks,
    const int32_t* __restrict__ seen, int cap, int window_len, int nblk, size_t total, int tri_mode, int n_prep,
    int gated, double max_e2_kept, double* __restrict__ cand, uint8_t* __restrict__ keep,
    int32_t* __restrict__ partial, uint8_t* __restrict__ reason, float* __restrict__ reproj_px) {
  __shared__ LmWaves S;
  const int tid = threadIdx.x;
  const int win = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int slot = blk * LM_THREADS + tid;
  const size_t idx = (size_t)win * cap + slot;
  // the same for every lane of the window: uniform addresses
  const double* tab = table + LM_VIEW_DOUBLES * ((size_t)window_len * win);
  double X[3] = {0.0, 0.0, 0.0};
  float px = 0.f;
  int why = LM_NO_WINDOW, obs = 0;
  if (gate[win] == LM_OK && slot < cap) {
    const int sn = lm_seen(seen[idx], window_len);
    why = LM_SHORT;
    if (sn >= 2) {
      const float* t = tracks + 2 * (size_t)window_len * idx;
      // rules 2-3: one view's rows at a time into the ten sums
      double a[4][4], rx[4], ry[4], h[4];
      lm_view_rows(tab, (double)t[0], (double)t[1], rx, ry);
      lm_normal_start(a, rx);
      lm_normal_add(a, ry);
      for (int k = 1; k < n_prep; k++) {
        if (lm_view_used(tri_mode, k, sn)) {
          lm_view_rows(tab + LM_VIEW_DOUBLES * k, (double)t[2 * k], (double)t[2 * k + 1], rx, ry);
          lm_normal_add(a, rx);
          lm_normal_add(a, ry);
        }
      }
      tri_smallest_eigenvector(a, h);
      why = LM_DEGENERATE;
      if (lm_quotient(h, X)) {
        // rules 5-6 over the observed views
        bool behind = tri_mode == LM_TRI_FIRST_TWO && !(X[2] > 0.0), bad = false;
        double max_e2 = 0.0;
        for (int k = 0; k < n_prep; k++) {
          if (k < sn) {
            const double* rec = tab + LM_VIEW_DOUBLES * k;
            if (tri_mode != LM_TRI_FIRST_TWO && !(lm_view_depth(rec, X) > 0.0)) behind = true;
            const double e2 = lm_view_e2(rec, X, (double)t[2 * k], (double)t[2 * k + 1]);
            if (!lm_finite(e2))
              bad = true;
            else if (e2 > max_e2)
              max_e2 = e2;
          }
        }
        px = lm_reproj_px(max_e2, bad);
        why = behind ? LM_BEHIND : (gated && (bad || max_e2 > max_e2_kept) ? LM_REPROJECTION : LM_KEPT);
        obs = why == LM_KEPT ? sn : 0;
      }
    }
  }
  const bool kept = why == LM_KEPT;
  if (slot < cap) {
#pragma unroll
    for (int k = 0; k < 3; k++) cand[k * total + idx] = X[k];
    keep[idx] = kept ? 1 : 0;
    reason[idx] = (uint8_t)why;
    reproj_px[idx] = px;
  }
  const int wave_kept = __popcll(__ballot(kept)), wave_obs = wave_sum(obs);
  int pa, pb, ta, tb;
  lm_cross_wave(S, wave_kept, wave_obs, &pa, &pb, &ta, &tb);
  if (tid == 0) {
    partial[2 * (size_t)blockIdx.x] = ta;
    partial[2 * (size_t)blockIdx.x + 1] = tb;
  }
}

__global__ __launch_bounds__(LM_THREADS) void k_lm_offsets(int n_windows, int window_len, int nblk,
                                                           const int32_t* __restrict__ partial,
                                                           const int32_t* __restrict__ gate,
                                                           int32_t* __restrict__ status,
                                                           int32_t* __restrict__ pose_off,
                                                           int32_t* __restrict__ pt_off,
                                                           int32_t* __restrict__ obs_off) {
  __shared__ LmWaves S;
  const int tid = threadIdx.x;
  int base_pt = 0, base_obs = 0;
  const int chunks = (n_windows + LM_THREADS - 1) / LM_THREADS;
  for (int c = 0; c < chunks; c++) {
    const int w = c * LM_THREADS + tid;
    int np = 0, no = 0;
    if (w < n_windows) {
      for (int b = 0; b < nblk; b++) {
        np += partial[2 * ((size_t)w * nblk + b)];
        no += partial[2 * ((size_t)w * nblk + b) + 1];
      }
      const int g = gate[w];
      status[w] = g == LM_OK && np == 0 ? LM_EMPTY : g;
    }
    const int ip = wave_scan_incl(np), io = wave_scan_incl(no);
    int pa, pb, ta, tb;
    lm_cross_wave(S, __builtin_amdgcn_readlane(ip, 63), __builtin_amdgcn_readlane(io, 63), &pa, &pb, &ta, &tb);
    if (w < n_windows) {
      pt_off[w] = base_pt + pa + ip - np;
      obs_off[w] = base_obs + pb + io - no;
      pose_off[w] = w * window_len;
    }
    base_pt += ta, base_obs += tb;
  }
  if (tid == 0) {
    pt_off[n_windows] = base_pt;
    obs_off[n_windows] = base_obs;
    pose_off[n_windows] = n_windows * window_len;
  }
}

__global__ __launch_bounds__(LM_THREADS) void k_lm_fill(const float* __restrict__ tracks,
                                                        const int32_t* __restrict__ seen, int cap, int window_len,
                                                        size_t total, const double* __restrict__ cand,
                                                        const uint8_t* __restrict__ keep,
                                                        const int32_t* __restrict__ pt_off,
                                                        const int32_t* __restrict__ obs_off,
                                                        double* __restrict__ points3, int32_t* __restrict__ rows,
                                                        uint8_t* __restrict__ opose, double* __restrict__ oxy,
                                                        int32_t* __restrict__ slot_of_point) {
  __shared__ LmWaves S;
  const int tid = threadIdx.x, win = blockIdx.x;
  const size_t po = (size_t)pt_off[win], oo = (size_t)obs_off[win];
  int32_t* row = rows + po + win;
  int base_pt = 0, base_obs = 0;
  const int chunks = (cap + LM_THREADS - 1) / LM_THREADS;
  for (int c = 0; c < chunks; c++) {
    const int slot = c * LM_THREADS + tid;
    const size_t idx = (size_t)win * cap + slot;
    bool kept = false;
    int obs = 0;
    if (slot < cap && keep[idx]) {
      kept = true;
      obs = lm_seen(seen[idx], window_len);
    }
    const unsigned long long mask = __ballot(kept);
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
    const int io = wave_scan_incl(obs);
    int pa, pb, ta, tb;
    lm_cross_wave(S, __popcll(mask), __builtin_amdgcn_readlane(io, 63), &pa, &pb, &ta, &tb);
    if (kept) {
      const int j = base_pt + pa + below, o = base_obs + pb + io - obs;
#pragma unroll
      for (int k = 0; k < 3; k++) points3[3 * (po + j) + k] = cand[k * total + idx];
      row[j] = o;
      slot_of_point[po + j] = slot;
      const float* t = tracks + 2 * (size_t)window_len * idx;
      for (int k = 0; k < window_len; k++) {
        if (k < obs) {
          opose[oo + o + k] = (uint8_t)k;
          oxy[2 * (oo + o + k)] = (double)t[2 * k];
          oxy[2 * (oo + o + k) + 1] = (double)t[2 * k + 1];
        }
      }
    }
    base_pt += ta, base_obs += tb;
  }
  if (tid == 0) row[base_pt] = base_obs;
}

}  // namespace

hipError_t orbx_launch_landmarks(hipStream_t s, const double* K9, const double* d_poses, const float* d_tracks,
                                 const int32_t* d_seen, int n_windows, int cap, int window_len, double* d_cand,
                                 uint8_t* d_keep, int32_t* d_partial, int32_t* d_gate, const OrbxLmBlock& out,
                                 const int32_t* d_pose_status) {
  if (n_windows < 1 || cap < 1 || cap > ORBX_BA_MAX_POINTS || window_len < 2 || window_len > ORBX_BA_MAX_POSES)
    return hipErrorInvalidValue;
  const int nblk = orbx_lm_blocks(cap);
  const size_t total = (size_t)n_windows * cap;
  if ((size_t)n_windows * nblk > 0x7fffffffu) return hipErrorInvalidValue;
  LmK9 K;
  for (int i = 0; i < 9; i++) K.k[i] = K9[i];
  hipLaunchKernelGGL(k_lm_triangulate, dim3((unsigned)(n_windows * nblk)), dim3(LM_THREADS), 0, s, K, d_poses,
                     d_tracks, d_seen, cap, window_len, nblk, total, d_cand, d_keep, d_partial, d_gate, d_pose_status);
  hipLaunchKernelGGL(k_lm_offsets, dim3(1), dim3(LM_THREADS), 0, s, n_windows, window_len, nblk, d_partial, d_gate,
                     out.status, out.pose_off, out.pt_off, out.obs_off);
  hipLaunchKernelGGL(k_lm_fill, dim3((unsigned)n_windows), dim3(LM_THREADS), 0, s, d_tracks, d_seen, cap, window_len,
                     total, d_cand, d_keep, out.pt_off, out.obs_off, out.points3, out.rows, out.opose, out.oxy,
                     out.slot_of_point);
  return hipGetLastError();
}

hipError_t orbx_launch_landmarks_views(hipStream_t s, const double* K9, const double* d_poses, const float* d_tracks,
                                       const int32_t* d_seen, int n_windows, int cap, int window_len, int tri_mode,
                                       double max_reproj_px, double* d_table, uint8_t* d_reason, float* d_reproj_px,
                                       double* d_cand, uint8_t* d_keep, int32_t* d_partial, int32_t* d_gate,
                                       const OrbxLmBlock& out, const int32_t* d_pose_status) {
  if (n_windows < 1 || cap < 1 || cap > ORBX_BA_MAX_POINTS || window_len < 2 || window_len > ORBX_BA_MAX_POSES ||
      tri_mode < LM_TRI_FIRST_TWO || tri_mode > LM_TRI_ALL_VIEWS || !(max_reproj_px >= 0.0))
    return hipErrorInvalidValue;
  const int nblk = orbx_lm_blocks(cap);
  const size_t total = (size_t)n_windows * cap;
  if ((size_t)n_windows * nblk > 0x7fffffffu) return hipErrorInvalidValue;
  LmK9 K;
  for (int i = 0; i < 9; i++) K.k[i] = K9[i];
  const int n_prep = lm_views_prepared(tri_mode, max_reproj_px, window_len);
  const unsigned view_blocks = (unsigned)(((size_t)n_windows * 8 + LM_THREADS - 1) / LM_THREADS);
  hipLaunchKernelGGL(k_lm_views, dim3(view_blocks), dim3(LM_THREADS), 0, s, K, d_poses, n_windows, window_len, n_prep,
                     d_pose_status, d_table, d_gate);
  hipLaunchKernelGGL(k_lm_triangulate_views, dim3((unsigned)(n_windows * nblk)), dim3(LM_THREADS), 0, s, d_table,
                     d_gate, d_tracks, d_seen, cap, window_len, nblk, total, tri_mode, n_prep,
                     max_reproj_px > 0.0 ? 1 : 0, max_reproj_px * max_reproj_px, d_cand, d_keep, d_partial, d_reason,
                     d_reproj_px);
  hipLaunchKernelGGL(k_lm_offsets, dim3(1), dim3(LM_THREADS), 0, s, n_windows, window_len, nblk, d_partial, d_gate,
                     out.status, out.pose_off, out.pt_off, out.obs_off);
  hipLaunchKernelGGL(k_lm_fill, dim3((unsigned)n_windows), dim3(LM_THREADS), 0, s, d_tracks, d_seen, cap, window_len,
                     total, d_cand, d_keep, out.pt_off, out.obs_off, out.points3, out.rows, out.opose, out.oxy,
                     out.slot_of_point);
  return hipGetLastError();
}
