// orbx_pose.hip -- batched essential-matrix RANSAC + recoverPose.
//
// Replaces, per consecutive frame pair,
//   cv::findEssentialMat(pts1, pts2, K, cv::RANSAC, prob, threshold, mask)   src/feature_matching.cpp:193
//   cv::recoverPose(E, pts1, pts2, K, R, t, mask)                             src/feature_matching.cpp:205
// (and src/feature_tracking.cpp:229,241).  Two launches per call:
//   k_pose_prep_batch / k_pose_prep_host: the pair's point list, normalised to double (rule 1);
//   k_pose_ransac: one workgroup (one wave) per pair -- RANSAC in chunks of POSE_CHUNK iterations, then the
//                  final mask and recoverPose.
// All per-sample arithmetic comes from orbx_pose_math.h, compiled with -ffp-contract=off, so each pair's
// result equals the sequential restatement (tests/cpp/pose_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_pose_math.h"
#include "orbx_wave.h"

namespace {

// samples solved per chunk: one per lane of the first half-wave, each in its own LDS workspace slice
// (POSE_WS doubles strided by POSE_CHUNK: 75.8 KB per workgroup, two workgroups per CU)
constexpr int POSE_CHUNK = 32;

__device__ __forceinline__ void pose_write_degenerate(OrbxPoseOut* o, uint8_t* mask, int n, int iters, int lane) {
  for (int p = lane; p < n; p += 64) mask[p] = 0;
  if (lane == 0) {
    for (int i = 0; i < 9; i++) {
      o->E[i] = 0.0;
      o->R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    o->t[0] = o->t[1] = o->t[2] = 0.0;
    o->inliers = 0;
    o->good = 0;
    o->iters = iters;
    o->pad = 0;
  }
}

// One wave per pair: the matches of pair p (query = frame p, train = frame p+1) in query order, compacted with
// the ordered wave scan, as normalised double coordinates.  Keypoints: int -> float -> double.
__global__ __launch_bounds__(64) void k_pose_prep_batch(int cap, const int32_t* __restrict__ counts,
                                                        const orbx_keypoint* __restrict__ kp,
                                                        const int32_t* __restrict__ match, double fx, double fy,
                                                        double cx, double cy, OrbxPosePt* __restrict__ pts,
                                                        int32_t* __restrict__ npts) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int nq = counts[pair];
  const size_t row = (size_t)pair * cap;
  int base = 0;
  for (int q0 = 0; q0 < nq; q0 += 64) {
    const int q = q0 + lane;
    const int m = q < nq ? match[row + q] : -1;
    const int has = m >= 0 ? 1 : 0;
    const int incl = wave_scan_incl(has);
    if (has) {
      const orbx_keypoint a = kp[row + q], b = kp[row + cap + m];
      OrbxPosePt o;
      o.x1 = ((double)(float)a.x - cx) / fx;
      o.y1 = ((double)(float)a.y - cy) / fy;
      o.x2 = ((double)(float)b.x - cx) / fx;
      o.y2 = ((double)(float)b.y - cy) / fy;
      pts[row + base + incl - 1] = o;
    }
    base += __builtin_amdgcn_readlane(incl, 63);
  }
  if (lane == 0) npts[pair] = base;
}

__global__ __launch_bounds__(256) void k_pose_prep_host(int n, const float* __restrict__ p1, const float* __restrict__ p2,
                                                        double fx, double fy, double cx, double cy,
                                                        OrbxPosePt* __restrict__ pts, int32_t* __restrict__ npts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    OrbxPosePt o;
    o.x1 = ((double)p1[2 * i] - cx) / fx;
    o.y1 = ((double)p1[2 * i + 1] - cy) / fy;
    o.x2 = ((double)p2[2 * i] - cx) / fx;
    o.y2 = ((double)p2[2 * i + 1] - cy) / fy;
    pts[i] = o;
  }
  if (i == 0) npts[0] = n;
}

__global__ __launch_bounds__(64) void k_pose_ransac(int cap, const OrbxPosePt* __restrict__ pts,
                                                    const int32_t* __restrict__ npts, double prob, float tf,
                                                    int max_iters, uint64_t seed, OrbxPoseOut* __restrict__ out,
                                                    uint8_t* __restrict__ mask) {
  __shared__ double ws[POSE_WS * POSE_CHUNK];
  __shared__ int s_nmod[POSE_CHUNK];
  __shared__ int s_cnt[POSE_CHUNK * POSE_MAX_MODELS];
  __shared__ double s_best[9];
  __shared__ int s_state[3];  // niters, best count, iterations run
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int n = npts[pair];
  const OrbxPosePt* P = pts + (size_t)pair * cap;
  uint8_t* M = mask + (size_t)pair * cap;
  OrbxPoseOut* o = out + pair;
  if (n < 5) {  // rule 7
    pose_write_degenerate(o, M, n, 0, lane);
    return;
  }
  if (lane == 0) {
    s_state[0] = max_iters;
    s_state[1] = 0;
    s_state[2] = 0;
  }
  __syncthreads();
  for (int base = 0;; base += POSE_CHUNK) {
    const int niters0 = s_state[0];
    if (base >= niters0) break;
    // 1. solve: lane l < POSE_CHUNK takes iteration base + l (iterations past the current niters are skipped)
    if (lane < POSE_CHUNK) {
      int nm = 0;
      const int it = base + lane;
      uint32_t idx[5];
      if (it < niters0 && pose_sample(seed, (uint32_t)it, (uint32_t)n, idx)) {
        double* w = ws + lane;
#pragma unroll
        for (int k = 0; k < 5; k++) {
          const OrbxPosePt q = P[idx[k]];
          pose_put_point<POSE_CHUNK>(w, k, q.x1, q.y1, q.x2, q.y2);
        }
        nm = pose_solve5<POSE_CHUNK>(w);
      }
      s_nmod[lane] = nm;
    }
    __syncthreads();
    // 2. score every model of the chunk over the pair's points (the wave strides the points)
    for (int l = 0; l < POSE_CHUNK; l++) {
      const int nm = s_nmod[l];
      for (int m = 0; m < nm; m++) {
        double E[9];
#pragma unroll
        for (int e = 0; e < 9; e++) E[e] = ws[(POSE_WS_MODELS + m * 9 + e) * POSE_CHUNK + l];
        int c = 0;
        for (int p = lane; p < n; p += 64) {
          const OrbxPosePt q = P[p];
          c += pose_sampson(E, q.x1, q.y1, q.x2, q.y2) <= tf ? 1 : 0;
        }
        c = wave_sum(c);
        if (lane == 0) s_cnt[l * POSE_MAX_MODELS + m] = c;
      }
    }
    __syncthreads();
    // 3. RANSACPointSetRegistrator::run's selection, in (iteration, model) order
    if (lane == 0) {
      int niters = s_state[0], best = s_state[1], i = base;
      for (; i < base + POSE_CHUNK && i < niters; i++) {
        const int l = i - base;
        for (int m = 0; m < s_nmod[l]; m++) {
          const int count = s_cnt[l * POSE_MAX_MODELS + m];
          if (count > (best > 4 ? best : 4)) {
            best = count;
            for (int e = 0; e < 9; e++) s_best[e] = ws[(POSE_WS_MODELS + m * 9 + e) * POSE_CHUNK + l];
            niters = pose_update_niters(prob, (double)(n - count) / n, niters);
          }
        }
      }
      s_state[0] = niters;
      s_state[1] = best;
      s_state[2] = i;
    }
    __syncthreads();
  }
  const int best = s_state[1], iters = s_state[2];
  if (best == 0) {
    pose_write_degenerate(o, M, n, iters, lane);
    return;
  }
  // 4. recoverPose on the best model's inliers
  double E[9], R1[9], R2[9], tu[3];
#pragma unroll
  for (int e = 0; e < 9; e++) E[e] = s_best[e];
  if (!pose_decompose(E, R1, R2, tu)) {
    pose_write_degenerate(o, M, n, iters, lane);
    return;
  }
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int p = lane; p < n; p += 64) {
    const OrbxPosePt q = P[p];
    if (pose_sampson(E, q.x1, q.y1, q.x2, q.y2) <= tf) {
      c0 += pose_point_good(R1, tu, 1.0, q.x1, q.y1, q.x2, q.y2) ? 1 : 0;
      c1 += pose_point_good(R2, tu, 1.0, q.x1, q.y1, q.x2, q.y2) ? 1 : 0;
      c2 += pose_point_good(R1, tu, -1.0, q.x1, q.y1, q.x2, q.y2) ? 1 : 0;
      c3 += pose_point_good(R2, tu, -1.0, q.x1, q.y1, q.x2, q.y2) ? 1 : 0;
    }
  }
  c0 = wave_sum(c0);
  c1 = wave_sum(c1);
  c2 = wave_sum(c2);
  c3 = wave_sum(c3);
  // the first candidate with the most good points (OpenCV's >= chain)
  int ch = 0, gc = c0;
  if (c1 > gc) ch = 1, gc = c1;
  if (c2 > gc) ch = 2, gc = c2;
  if (c3 > gc) ch = 3, gc = c3;
  const double* Rc = (ch & 1) ? R2 : R1;
  const double sg = ch >= 2 ? -1.0 : 1.0;
  for (int p = lane; p < n; p += 64) {
    const OrbxPosePt q = P[p];
    M[p] = (pose_sampson(E, q.x1, q.y1, q.x2, q.y2) <= tf && pose_point_good(Rc, tu, sg, q.x1, q.y1, q.x2, q.y2)) ? 1 : 0;
  }
  if (lane == 0) {
    for (int i = 0; i < 9; i++) {
      o->E[i] = E[i];
      o->R[i] = Rc[i];
    }
    for (int i = 0; i < 3; i++) o->t[i] = sg * tu[i];
    o->inliers = best;
    o->good = gc;
    o->iters = iters;
    o->pad = 0;
  }
}

}  // namespace

hipError_t orbx_launch_pose_prep_batch(hipStream_t s, int npairs, int cap, const int32_t* d_counts,
                                       const orbx_keypoint* d_kp, const int32_t* d_match, const double* K,
                                       OrbxPosePt* d_pts, int32_t* d_npts) {
  if (npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pose_prep_batch, dim3(npairs), dim3(64), 0, s, cap, d_counts, d_kp, d_match, K[0], K[4], K[2],
                     K[5], d_pts, d_npts);
  return hipGetLastError();
}

hipError_t orbx_launch_pose_prep_host(hipStream_t s, int n, const float* d_p1, const float* d_p2, const double* K,
                                      OrbxPosePt* d_pts, int32_t* d_npts) {
  const int blocks = n > 0 ? (n + 255) / 256 : 1;
  hipLaunchKernelGGL(k_pose_prep_host, dim3(blocks), dim3(256), 0, s, n, d_p1, d_p2, K[0], K[4], K[2], K[5], d_pts,
                     d_npts);
  return hipGetLastError();
}

hipError_t orbx_launch_pose_ransac(hipStream_t s, int npairs, int cap, const OrbxPosePt* d_pts, const int32_t* d_npts,
                                   const double* K, double prob, double threshold, int max_iters, uint64_t seed,
                                   OrbxPoseOut* d_out, uint8_t* d_mask) {
  if (npairs <= 0) return hipSuccess;
  // findEssentialMat: threshold /= (fx + fy) / 2; computeError compares against (float)(thr * thr)
  const double thr = threshold / ((K[0] + K[4]) / 2.0);
  const float tf = (float)(thr * thr);
  hipLaunchKernelGGL(k_pose_ransac, dim3(npairs), dim3(64), 0, s, cap, d_pts, d_npts, prob, tf, max_iters, seed, d_out,
                     d_mask);
  return hipGetLastError();
}
