// orbx_stitch.hip -- overlapping tracked windows joined into one trajectory on the device.
//
// Replaces, for a stream of n_windows windows per call, what the reference does between two solves
// (src/with_bundle_adjustment.cpp:203 and :234-249): cur_pose = prev_pose * T.inv(), cur_pose = pose_window.back()
// after the solve, est_path rewritten from pose_window.  Every window was chained, solved and gated in a frame of its
// own; here they are put behind one another:
//   k_st_scale0   one lane per window: the scale of pair 0 of window w, read from pair `stride` of window w - 1 of the
//                 tracks-pose block in place, into the scale0 section of the chain's input block
//   k_st_links    one lane per window: rel(w, stride), the two baselines and the broken flag
//   k_st_fold     ONE lane walks the windows: the left fold of the links.  Floating-point matrix products are not
//                 associative and the results have to equal a sequential loop bit for bit, so this is no tree scan
//   k_st_apply    one lane per stream frame: the owner's anchor times the frame's motion inside the window; owner
// All are latency-sized: serial binary64 on a few lanes.  All arithmetic comes from orbx_st_math.h, compiled with
// -ffp-contract=off, so every result equals the sequential restatement (tests/cpp/st_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "orbx_internal.h"
#include "orbx_st_math.h"

namespace {

constexpr int ST_THREADS = 64;
static_assert(sizeof(OrbxScaleOut) == 2 * sizeof(double) && offsetof(OrbxScaleOut, scale) == 0, "OrbxScaleOut");

__global__ __launch_bounds__(ST_THREADS) void k_st_scale0(int n_windows, int window_len, int stride,
                                                          double scale0_first, const OrbxScaleOut* __restrict__ scale,
                                                          double* __restrict__ scale0) {
  const int w = blockIdx.x * ST_THREADS + threadIdx.x;
  if (w >= n_windows) return;
  double s = scale0_first;
  if (w > 0) {
    const long long p = st_scale0_pair(w, window_len, stride);
    s = p >= 0 ? scale[p].scale : 1.0;
  }
  scale0[w] = s;
}

__global__ __launch_bounds__(ST_THREADS) void k_st_links(int n_windows, int window_len, int stride,
                                                         const double* __restrict__ poses4x4,
                                                         double* __restrict__ links, int32_t* __restrict__ broken) {
  const int w = blockIdx.x * ST_THREADS + threadIdx.x;
  if (w >= n_windows) return;
  double link[ST_LINK_DOUBLES];
  broken[w] = st_link(poses4x4 + 16 * (size_t)w * window_len, window_len, stride, link);
#pragma unroll
  for (int i = 0; i < ST_LINK_DOUBLES; i++) links[(size_t)ST_LINK_DOUBLES * w + i] = link[i];
}

__global__ __launch_bounds__(ST_THREADS) void k_st_fold(int n_windows, const double* __restrict__ links,
                                                        const int32_t* __restrict__ broken,
                                                        const double* __restrict__ T_start, int align_scale,
                                                        double* __restrict__ anchors4x4, double* __restrict__ lambda,
                                                        int32_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double G[16], Lam, b_link_prev = 0.0;
  st_fold_begin(T_start, G, &Lam);
  for (int w = 0; w < n_windows; w++) {
    double link[ST_LINK_DOUBLES], anchor[16], lam;
#pragma unroll
    for (int i = 0; i < ST_LINK_DOUBLES; i++) link[i] = links[(size_t)ST_LINK_DOUBLES * w + i];
    status[w] = st_fold_step(w, link, broken[w], b_link_prev, align_scale, G, &Lam, anchor, &lam);
    b_link_prev = link[13];
#pragma unroll
    for (int i = 0; i < 16; i++) anchors4x4[16 * (size_t)w + i] = anchor[i];
    lambda[w] = lam;
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_st_apply(int n_frames, int n_windows, int window_len, int stride,
                                                         const double* __restrict__ poses4x4,
                                                         const double* __restrict__ anchors4x4,
                                                         const double* __restrict__ lambda,
                                                         const int32_t* __restrict__ status,
                                                         double* __restrict__ trajectory4x4,
                                                         int32_t* __restrict__ owner) {
  const int f = blockIdx.x * ST_THREADS + threadIdx.x;
  if (f >= n_frames) return;
  double T[16];
  owner[f] = st_apply(f, n_windows, window_len, stride, poses4x4, anchors4x4, lambda, status, T);
#pragma unroll
  for (int i = 0; i < 16; i++) trajectory4x4[16 * (size_t)f + i] = T[i];
}

unsigned st_blocks(int n) { return (unsigned)((n + ST_THREADS - 1) / ST_THREADS); }

}  // namespace

hipError_t orbx_launch_st_scale0(hipStream_t s, int n_windows, int window_len, int stride, double scale0_first,
                                 const OrbxScaleOut* d_scale, double* d_scale0) {
  if (n_windows < 1 || window_len < 2 || stride < 1 || stride > window_len - 1) return hipErrorInvalidValue;
  if ((unsigned long long)n_windows * window_len > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_st_scale0, dim3(st_blocks(n_windows)), dim3(ST_THREADS), 0, s, n_windows, window_len, stride,
                     scale0_first, d_scale, d_scale0);
  return hipGetLastError();
}

hipError_t orbx_launch_stitch(hipStream_t s, int n_windows, int window_len, int stride, const double* d_poses4x4,
                              const double* d_T_start, int align_scale, double* d_links, int32_t* d_broken,
                              double* d_trajectory4x4, int32_t* d_owner, double* d_anchors4x4, double* d_lambda,
                              int32_t* d_status) {
  const int n_frames = st_frames(n_windows, window_len, stride);
  if (n_frames < 1 || (unsigned long long)n_windows * window_len > 0x7fffffffull / 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_st_links, dim3(st_blocks(n_windows)), dim3(ST_THREADS), 0, s, n_windows, window_len, stride,
                     d_poses4x4, d_links, d_broken);
  hipLaunchKernelGGL(k_st_fold, dim3(1), dim3(ST_THREADS), 0, s, n_windows, d_links, d_broken, d_T_start, align_scale,
                     d_anchors4x4, d_lambda, d_status);
  hipLaunchKernelGGL(k_st_apply, dim3(st_blocks(n_frames)), dim3(ST_THREADS), 0, s, n_frames, n_windows, window_len,
                     stride, d_poses4x4, d_anchors4x4, d_lambda, d_status, d_trajectory4x4, d_owner);
  return hipGetLastError();
}
