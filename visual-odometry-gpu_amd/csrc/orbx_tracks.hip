// orbx_tracks.hip -- pose and scale of tracked frame pairs from LK windows.
//
// Replaces, per consecutive frame pair of a tracked window, the host side of the reference's tracking loop:
//   the "remove lost tracks" compaction of track_optical_flow          src/feature_tracking.cpp:182-192
//   the point lists handed to get_pose and get_scale                    src/feature_tracking.cpp:66-93
// The tracks block of k_lk_track_windows (tracks_xy[w][slot][k][2], seen[w][slot]) stays on the device.  Kernels:
//   k_tracks_prep:        one workgroup per (window, pair) -- the slots that survive the pair, compacted in slot order
//                         (ballot + prefix, no atomics), as the normalised doubles k_pose_ransac reads;
//   k_tracks_triangulate: one workgroup per pair, one lane per list position, P1 / P2 once per workgroup.
// The pose is k_pose_ransac and the scale is k_scale_join (orbx_scale.hip) with one chain per window and the slot
// lists as its index arrays; neither is restated here.  All per-point arithmetic comes from orbx_tri_math.h, compiled
// with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"
#include "orbx_tri_math.h"
#include "orbx_wave.h"

namespace {

constexpr int TRK_THREADS = 256;

struct TrkK {
  double K[9];
};

// Pair k of window w: the list is the slots with seen >= k + 2 (seen clamped to [0, window_len]) in ascending slot
// order; point 1 is the slot's entry k, point 2 its entry k + 1, floats widened to double.
__global__ __launch_bounds__(TRK_THREADS) void k_tracks_prep(int cap, int window_len, const float* __restrict__ tracks,
                                                             const int32_t* __restrict__ seen, double fx, double fy,
                                                             double cx, double cy, OrbxPosePt* __restrict__ pts,
                                                             int32_t* __restrict__ npts, int32_t* __restrict__ slot_of,
                                                             uint8_t* __restrict__ mask, float* __restrict__ xyz,
                                                             uint8_t* __restrict__ valid) {
  __shared__ int s_wave[TRK_THREADS / 64];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int w = pair / (window_len - 1), k = pair - w * (window_len - 1);
  const size_t row = (size_t)pair * cap, wrow = (size_t)w * cap;
  int base = 0;
  for (int s0 = 0; s0 < cap; s0 += TRK_THREADS) {
    const int slot = s0 + tid;
    const int has = (slot < cap && lm_seen(seen[wrow + slot], window_len) >= k + 2) ? 1 : 0;
    int total;
    const int pos = base + block_scan_excl<TRK_THREADS>(has, s_wave, &total);
    if (has) {
      const float* t = tracks + 2 * ((wrow + slot) * window_len + k);
      OrbxPosePt o;
      o.x1 = ((double)t[0] - cx) / fx;
      o.y1 = ((double)t[1] - cy) / fy;
      o.x2 = ((double)t[2] - cx) / fx;
      o.y2 = ((double)t[3] - cy) / fy;
      pts[row + pos] = o;
      slot_of[row + pos] = slot;
    }
    base += total;
  }
  // everything past the list is 0 (k_pose_ransac and k_tracks_triangulate write [0, n) only)
  for (int i = base + tid; i < cap; i += TRK_THREADS) {
    slot_of[row + i] = 0;
    mask[row + i] = 0;
    valid[row + i] = 0;
    xyz[3 * (row + i) + 0] = 0.f;
    xyz[3 * (row + i) + 1] = 0.f;
    xyz[3 * (row + i) + 2] = 0.f;
  }
  if (tid == 0) npts[pair] = base;
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_triangulate(int cap, int window_len,
                                                                    const float* __restrict__ tracks,
                                                                    const int32_t* __restrict__ npts,
                                                                    const int32_t* __restrict__ slot_of,
                                                                    const OrbxPoseOut* __restrict__ pose, TrkK Kc,
                                                                    float* __restrict__ xyz,
                                                                    uint8_t* __restrict__ valid) {
  __shared__ double s_P[24];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int w = pair / (window_len - 1), k = pair - w * (window_len - 1);
  const size_t row = (size_t)pair * cap, wrow = (size_t)w * cap;
  const int n = min(npts[pair], cap);
  if (tid == 0) tri_projections(Kc.K, pose[pair].R, pose[pair].t, s_P, s_P + 12);
  __syncthreads();
  for (int i = tid; i < n; i += TRK_THREADS) {
    const int slot = slot_of[row + i];
    const float* t = tracks + 2 * ((wrow + slot) * window_len + k);
    float X[3];
    const bool ok = tri_point(s_P, s_P + 12, (double)t[0], (double)t[1], (double)t[2], (double)t[3], X);
    xyz[3 * (row + i) + 0] = X[0];
    xyz[3 * (row + i) + 1] = X[1];
    xyz[3 * (row + i) + 2] = X[2];
    valid[row + i] = ok ? 1 : 0;
  }
}

}  // namespace

hipError_t orbx_launch_tracks_prep(hipStream_t s, int n_windows, int cap, int window_len, const float* d_tracks,
                                   const int32_t* d_seen, const double* K, OrbxPosePt* d_pts, int32_t* d_npts,
                                   int32_t* d_slot_of, uint8_t* d_mask, float* d_xyz, uint8_t* d_valid) {
  if (n_windows <= 0) return hipSuccess;
  if (cap < 1 || window_len < 2) return hipErrorInvalidValue;
  const unsigned npairs = (unsigned)n_windows * (unsigned)(window_len - 1);
  hipLaunchKernelGGL(k_tracks_prep, dim3(npairs), dim3(TRK_THREADS), 0, s, cap, window_len, d_tracks, d_seen, K[0],
                     K[4], K[2], K[5], d_pts, d_npts, d_slot_of, d_mask, d_xyz, d_valid);
  return hipGetLastError();
}

hipError_t orbx_launch_tracks_triangulate(hipStream_t s, int n_windows, int cap, int window_len, const float* d_tracks,
                                          const int32_t* d_npts, const int32_t* d_slot_of, const OrbxPoseOut* d_pose,
                                          const double* K, float* d_xyz, uint8_t* d_valid) {
  if (n_windows <= 0) return hipSuccess;
  if (cap < 1 || window_len < 2) return hipErrorInvalidValue;
  const unsigned npairs = (unsigned)n_windows * (unsigned)(window_len - 1);
  TrkK Kc;
  for (int i = 0; i < 9; i++) Kc.K[i] = K[i];
  hipLaunchKernelGGL(k_tracks_triangulate, dim3(npairs), dim3(TRK_THREADS), 0, s, cap, window_len, d_tracks, d_npts,
                     d_slot_of, d_pose, Kc, d_xyz, d_valid);
  return hipGetLastError();
}
