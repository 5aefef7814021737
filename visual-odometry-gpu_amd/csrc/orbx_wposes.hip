// orbx_wposes.hip -- the poses of many tracked windows chained on the device from their pair motions, and the
// write-back gate behind their bundle adjustment.
//
// Replaces, for n_windows windows per call, the host code between orbx_tracks_pose_device and
// orbx_landmarks_build_device (src/with_bundle_adjustment.cpp:196-208 and :615-628) and the one behind
// orbx_bundle_adjust_landmarks_device (:683-718):
//   k_window_poses    one lane per window (the chain is sequential in the frame, and a window has at most 8): reads
//                     R, t and scale from the tracks-pose block in place, writes the window's 6-double blocks, its
//                     camera -> world 4x4 poses and its status
//   k_ba_write_back   one lane per (window, pose): the block after the solve against the block as built, the solve's
//                     summary; writes the gated camera -> world 4x4 and the updated flag
// Both are latency-sized: a few hundred lanes of serial binary64.  All arithmetic comes from orbx_wp_math.h, compiled
// with -ffp-contract=off, so every result equals the sequential restatement (tests/cpp/wp_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "orbx_internal.h"
#include "orbx_wp_math.h"

namespace {

constexpr int WP_THREADS = 64;
// the strides, in doubles, with which wp_chain_window walks the tracks-pose block
static_assert(sizeof(OrbxPoseOut) % sizeof(double) == 0 && offsetof(OrbxPoseOut, R) == 9 * sizeof(double) &&
                  offsetof(OrbxPoseOut, t) == 18 * sizeof(double),
              "OrbxPoseOut: E | R | t in doubles");
static_assert(sizeof(OrbxScaleOut) == 2 * sizeof(double) && offsetof(OrbxScaleOut, scale) == 0, "OrbxScaleOut");
constexpr int POSE_STRIDE = (int)(sizeof(OrbxPoseOut) / sizeof(double));
constexpr int SCALE_STRIDE = (int)(sizeof(OrbxScaleOut) / sizeof(double));
static_assert(sizeof(BaSummary) == 32, "BaSummary = orbx_ba_summary");

__global__ __launch_bounds__(WP_THREADS) void k_window_poses(int n_windows, int window_len,
                                                             const OrbxPoseOut* __restrict__ pose,
                                                             const OrbxScaleOut* __restrict__ scale,
                                                             const double* __restrict__ T0,
                                                             const double* __restrict__ scale0,
                                                             double* __restrict__ poses6,
                                                             double* __restrict__ poses4x4,
                                                             int32_t* __restrict__ status) {
  const int w = blockIdx.x * WP_THREADS + threadIdx.x;
  if (w >= n_windows) return;
  const size_t pair0 = (size_t)w * (window_len - 1), frame0 = (size_t)w * window_len;
  const double* p = reinterpret_cast<const double*>(pose + pair0);
  const double* s = reinterpret_cast<const double*>(scale + pair0);
  status[w] = wp_chain_window(T0 + 16 * (size_t)w, p + 9, POSE_STRIDE, p + 18, POSE_STRIDE, s, SCALE_STRIDE, scale0[w],
                              window_len, poses4x4 + 16 * frame0, poses6 + 6 * frame0);
}

__global__ __launch_bounds__(WP_THREADS) void k_ba_write_back(int n_poses, int window_len,
                                                              const double* __restrict__ solved6,
                                                              const double* __restrict__ built6,
                                                              const BaSummary* __restrict__ summaries, double max_rot,
                                                              double max_trans, double* __restrict__ poses4x4,
                                                              uint8_t* __restrict__ updated) {
  const int i = blockIdx.x * WP_THREADS + threadIdx.x;
  if (i >= n_poses) return;
  double T[16], angle, dist;
  const int up = wp_gate(solved6 + 6 * (size_t)i, built6 + 6 * (size_t)i, summaries[i / window_len].termination,
                         max_rot, max_trans, T, &angle, &dist);
#pragma unroll
  for (int k = 0; k < 16; k++) poses4x4[16 * (size_t)i + k] = T[k];
  updated[i] = (uint8_t)up;
}

}  // namespace

hipError_t orbx_launch_window_poses(hipStream_t s, int n_windows, int window_len, const OrbxPoseOut* d_pose,
                                    const OrbxScaleOut* d_scale, const double* d_T0, const double* d_scale0,
                                    double* d_poses6, double* d_poses4x4, int32_t* d_status) {
  if (n_windows < 1 || window_len < 2 || window_len > ORBX_BA_MAX_POSES) return hipErrorInvalidValue;
  if ((unsigned long long)n_windows * window_len > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_window_poses, dim3((unsigned)((n_windows + WP_THREADS - 1) / WP_THREADS)), dim3(WP_THREADS), 0,
                     s, n_windows, window_len, d_pose, d_scale, d_T0, d_scale0, d_poses6, d_poses4x4, d_status);
  return hipGetLastError();
}

hipError_t orbx_launch_ba_write_back(hipStream_t s, int n_windows, int window_len, const double* d_solved6,
                                     const double* d_built6, const void* d_summaries, double max_rot,
                                     double max_trans, double* d_poses4x4, uint8_t* d_updated) {
  if (n_windows < 1 || window_len < 2 || window_len > ORBX_BA_MAX_POSES) return hipErrorInvalidValue;
  if ((unsigned long long)n_windows * window_len > 0x7fffffffull) return hipErrorInvalidValue;
  const int n_poses = n_windows * window_len;
  hipLaunchKernelGGL(k_ba_write_back, dim3((unsigned)((n_poses + WP_THREADS - 1) / WP_THREADS)), dim3(WP_THREADS), 0, s,
                     n_poses, window_len, d_solved6, d_built6, (const BaSummary*)d_summaries, max_rot, max_trans,
                     d_poses4x4, d_updated);
  return hipGetLastError();
}
