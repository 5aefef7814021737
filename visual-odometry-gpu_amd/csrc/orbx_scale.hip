// orbx_scale.hip -- batched triangulation and relative scale.
//
// Replaces, per consecutive frame pair, the reference's get_scale
//   cv::triangulatePoints(P1, P2, pts1_T, pts2_T, points_4d_h) + X/w                src/feature_matching.cpp:216-245
//   median of |prev_i - prev_i-1| / (|cur_i - cur_i-1| + 1e-6), clamped to [0.1, 5]  src/feature_matching.cpp:248-274
// (and src/feature_tracking.cpp:244-310; the join of src/feature_tracking_scale.py:127-164).  Kernels:
//   k_triangulate_batch / k_triangulate_host: one lane per correspondence, the 4x4 DLT by fixed-sweep Jacobi;
//   k_scale_join: one workgroup per pair -- joins the pair's matches with its predecessor's on the shared frame's
//                 keypoint index (inverse map in LDS), ratios into LDS, exact selection by rank counting;
//   k_scale_aligned: the same selection over two index-aligned host lists.
// All per-point arithmetic comes from orbx_tri_math.h, compiled with -ffp-contract=off, so every result equals the
// sequential restatement (tests/cpp/scale_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <atomic>

#include "orbx_internal.h"
#include "orbx_tri_math.h"
#include "orbx_wave.h"

namespace {

constexpr int SCALE_THREADS = 256;
// key of an index that contributes no ratio: above every ratio's bit pattern (ratios are finite and >= 0, so
// their bit patterns order like their values)
constexpr u64 SCALE_NO_RATIO = ~0ull;

// Rule 3's selection: keys[0, n) in LDS hold the ratios' bit patterns (SCALE_NO_RATIO where an index contributes
// none), r of them are ratios.  The element at sorted position r / 2 is the one with at most r / 2 keys below it
// and more than r / 2 keys not above it; equal keys are the same double, so whichever thread finds it writes the
// same bits.
__device__ __forceinline__ void scale_select(const u64* keys, int n, int r, double* s_median) {
  const int k = r / 2;
  for (int i = threadIdx.x; i < n; i += SCALE_THREADS) {
    const u64 key = keys[i];
    if (key == SCALE_NO_RATIO) continue;
    int less = 0, leq = 0;
    for (int j = 0; j < n; j++) {
      const u64 o = keys[j];
      less += o < key ? 1 : 0;
      leq += o <= key ? 1 : 0;
    }
    if (less <= k && k < leq) *s_median = pose_u2d(key);
  }
}

struct TriK {
  double K[9];
};

// One workgroup per pair: the matches of pair p (query = frame p, train = frame p + 1) compacted in query order
// (as k_pose_prep_batch does, here across four waves), then one lane per correspondence.  Dynamic LDS: cap ints.
__global__ __launch_bounds__(SCALE_THREADS) void k_triangulate_batch(
    int cap, const int32_t* __restrict__ counts, const orbx_keypoint* __restrict__ kp, const int32_t* __restrict__ match,
    const OrbxPoseOut* __restrict__ pose, TriK Kc, float* __restrict__ xyz, uint8_t* __restrict__ valid,
    int32_t* __restrict__ mq, int32_t* __restrict__ mt, int32_t* __restrict__ npts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tri_lds[];
  int32_t* s_q = (int32_t*)tri_lds;  // compact position -> query index
  __shared__ double s_P[24];
  __shared__ int s_wave[SCALE_THREADS / 64];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int nq = min(counts[pair], cap);
  const size_t row = (size_t)pair * cap;
  if (tid == 0) tri_projections(Kc.K, pose[pair].R, pose[pair].t, s_P, s_P + 12);
  int base = 0;
  for (int q0 = 0; q0 < nq; q0 += SCALE_THREADS) {
    const int q = q0 + tid;
    const int m = q < nq ? match[row + q] : -1;
    const int has = (m >= 0 && m < cap) ? 1 : 0;  // never index the next frame's slots with anything else
    int total;
    const int pos = base + block_scan_excl<SCALE_THREADS>(has, s_wave, &total);
    if (has) s_q[pos] = q;
    base += total;
  }
  __syncthreads();
  const int n = base;
  for (int i = tid; i < n; i += SCALE_THREADS) {
    const int q = s_q[i];
    const int m = match[row + q];
    const orbx_keypoint a = kp[row + q], b = kp[row + cap + m];
    float X[3];
    const bool ok = tri_point(s_P, s_P + 12, (double)(float)a.x, (double)(float)a.y, (double)(float)b.x,
                              (double)(float)b.y, X);
    xyz[3 * (row + i) + 0] = X[0];
    xyz[3 * (row + i) + 1] = X[1];
    xyz[3 * (row + i) + 2] = X[2];
    valid[row + i] = ok ? 1 : 0;
    mq[row + i] = q;
    mt[row + i] = m;
  }
  if (tid == 0) npts[pair] = n;
}

struct TriP {
  double P[24];  // P1, P2
};

__global__ __launch_bounds__(SCALE_THREADS) void k_triangulate_host(int n, const float* __restrict__ p1,
                                                                    const float* __restrict__ p2, TriP Pc,
                                                                    float* __restrict__ xyz, uint8_t* __restrict__ valid) {
  const int i = blockIdx.x * SCALE_THREADS + threadIdx.x;
  if (i >= n) return;
  float X[3];
  const bool ok = tri_point(Pc.P, Pc.P + 12, (double)p1[2 * i], (double)p1[2 * i + 1], (double)p2[2 * i],
                            (double)p2[2 * i + 1], X);
  xyz[3 * i + 0] = X[0];
  xyz[3 * i + 1] = X[1];
  xyz[3 * i + 2] = X[2];
  valid[i] = ok ? 1 : 0;
}

// One workgroup per pair p.  The pairs form chains of `chain` consecutive pairs (the frames of a batch: one chain of
// all pairs; the frames of tracked windows: one chain per window).  The first pair of a chain has no predecessor:
// scale 1.0, no triplets.  Dynamic LDS, 16 bytes per slot
// of `cap`: [keys: cap u64 | trip_i: cap ints | trip_j: cap ints]; the inverse map (cap ints) lives in the keys'
// space until the triplets are listed.
__global__ __launch_bounds__(SCALE_THREADS) void k_scale_join(int cap, int chain, const int32_t* __restrict__ npts,
                                                              const int32_t* __restrict__ mq,
                                                              const int32_t* __restrict__ mt,
                                                              const float* __restrict__ xyz,
                                                              const uint8_t* __restrict__ valid,
                                                              const OrbxPoseOut* __restrict__ pose,
                                                              OrbxScaleOut* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char join_lds[];
  u64* s_key = (u64*)join_lds;
  int32_t* s_inv = (int32_t*)join_lds;
  int32_t* s_ti = (int32_t*)(join_lds + (size_t)cap * 8);
  int32_t* s_tj = s_ti + cap;
  __shared__ int s_wave[SCALE_THREADS / 64];
  __shared__ int s_used;
  __shared__ double s_median;
  const int pair = blockIdx.x, tid = threadIdx.x;
  if (pair % chain == 0) {
    if (tid == 0) {
      out[pair].scale = 1.0;
      out[pair].triplets = 0;
      out[pair].ratios_used = 0;
    }
    return;
  }
  const int n_prev = min(npts[pair - 1], cap), n_cur = min(npts[pair], cap);
  const size_t prow = (size_t)(pair - 1) * cap, crow = (size_t)pair * cap;
  // 1. frame-`pair` keypoint index -> position in the previous pair's list; the largest position (= the largest
  //    query index) wins
  for (int m = tid; m < cap; m += SCALE_THREADS) s_inv[m] = -1;
  if (tid == 0) {
    s_used = 0;
    s_median = 1.0;
  }
  __syncthreads();
  for (int i = tid; i < n_prev; i += SCALE_THREADS) {
    const int m = mt[prow + i];
    if (m >= 0 && m < cap) atomicMax(&s_inv[m], i);
  }
  __syncthreads();
  // 2. the triplets, in ascending frame-`pair` index = this pair's query order
  int nt = 0;
  for (int j0 = 0; j0 < n_cur; j0 += SCALE_THREADS) {
    const int j = j0 + tid;
    int i = -1;
    if (j < n_cur) {
      const int q = mq[crow + j];
      i = (q >= 0 && q < cap) ? s_inv[q] : -1;
    }
    const int has = i >= 0 ? 1 : 0;
    int total;
    const int pos = nt + block_scan_excl<SCALE_THREADS>(has, s_wave, &total);
    if (has) {
      s_ti[pos] = i;
      s_tj[pos] = j;
    }
    nt += total;
  }
  __syncthreads();  // the inverse map is dead: its space becomes the keys'
  // 3. ratios of consecutive triplets
  double R[9], t[3];
#pragma unroll
  for (int e = 0; e < 9; e++) R[e] = pose[pair - 1].R[e];
#pragma unroll
  for (int e = 0; e < 3; e++) t[e] = pose[pair - 1].t[e];
  int used = 0;
  for (int k = tid; k < nt; k += SCALE_THREADS) {
    u64 key = SCALE_NO_RATIO;
    if (k >= 1) {
      const int i1 = s_ti[k], i0 = s_ti[k - 1], j1 = s_tj[k], j0 = s_tj[k - 1];
      if (valid[prow + i1] && valid[prow + i0] && valid[crow + j1] && valid[crow + j0]) {
        float a1[3], a0[3];
        tri_transform(R, t, xyz + 3 * (prow + i1), a1);
        tri_transform(R, t, xyz + 3 * (prow + i0), a0);
        const double ratio = tri_ratio(a1, a0, xyz + 3 * (crow + j1), xyz + 3 * (crow + j0));
        if (tri_ratio_ok(ratio)) {
          key = pose_d2u(ratio);
          used++;
        }
      }
    }
    s_key[k] = key;
  }
  used = wave_sum(used);
  if ((tid & 63) == 0 && used) atomicAdd(&s_used, used);
  __syncthreads();
  // 4. the upper median
  const int r = s_used;
  if (r > 0) scale_select(s_key, nt, r, &s_median);
  __syncthreads();
  if (tid == 0) {
    out[pair].scale = r > 0 ? tri_scale_clamp(s_median) : 1.0;
    out[pair].triplets = nt;
    out[pair].ratios_used = r;
  }
}

// Rule 3 on two index-aligned lists (one workgroup).  A NULL valid array: all valid.  Dynamic LDS: m u64.
__global__ __launch_bounds__(SCALE_THREADS) void k_scale_aligned(int n_prev, int n_cur,
                                                                 const float* __restrict__ prev,
                                                                 const uint8_t* __restrict__ prev_valid,
                                                                 const float* __restrict__ cur,
                                                                 const uint8_t* __restrict__ cur_valid,
                                                                 OrbxScaleOut* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aligned_lds[];
  u64* s_key = (u64*)aligned_lds;
  __shared__ int s_used;
  __shared__ double s_median;
  const int tid = threadIdx.x;
  const int m = min(n_prev, n_cur);
  if (tid == 0) {
    s_used = 0;
    s_median = 1.0;
  }
  __syncthreads();
  int used = 0;
  for (int k = tid; k < m; k += SCALE_THREADS) {
    u64 key = SCALE_NO_RATIO;
    if (k >= 1) {
      const bool ok = (!prev_valid || (prev_valid[k] && prev_valid[k - 1])) && (!cur_valid || (cur_valid[k] && cur_valid[k - 1]));
      if (ok) {
        const double ratio = tri_ratio(prev + 3 * k, prev + 3 * (k - 1), cur + 3 * k, cur + 3 * (k - 1));
        if (tri_ratio_ok(ratio)) {
          key = pose_d2u(ratio);
          used++;
        }
      }
    }
    s_key[k] = key;
  }
  used = wave_sum(used);
  if ((tid & 63) == 0 && used) atomicAdd(&s_used, used);
  __syncthreads();
  const int r = s_used;
  if (r > 0) scale_select(s_key, m, r, &s_median);
  __syncthreads();
  if (tid == 0) {
    out->scale = r > 0 ? tri_scale_clamp(s_median) : 1.0;
    out->triplets = 0;
    out->ratios_used = r;
  }
}

// Dynamic LDS above 48 KB has to be granted to the kernel once per device; the largest size granted is remembered
// (one instance of this template, and so of `granted`, per kernel), so a steady stream of launches asks only once.
template <class F>
hipError_t allow_lds(F kernel, size_t bytes) {
  constexpr int MAX_DEV = 64;
  static std::atomic<size_t> granted[MAX_DEV];
  if (bytes > ORBX_SCALE_LDS_MAX) return hipErrorInvalidValue;
  if (bytes <= 48 * 1024) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < MAX_DEV;
  if (known && granted[dev].load(std::memory_order_relaxed) >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          ORBX_SCALE_LDS_MAX);
  if (e == hipSuccess && known) granted[dev].store(ORBX_SCALE_LDS_MAX, std::memory_order_relaxed);
  return e;
}

}  // namespace

hipError_t orbx_launch_triangulate_batch(hipStream_t s, int npairs, int cap, const int32_t* d_counts,
                                         const orbx_keypoint* d_kp, const int32_t* d_match, const OrbxPoseOut* d_pose,
                                         const double* K, float* d_xyz, uint8_t* d_valid, int32_t* d_mq, int32_t* d_mt,
                                         int32_t* d_npts) {
  if (npairs <= 0) return hipSuccess;
  const size_t lds = (size_t)cap * 4;
  hipError_t e = allow_lds(k_triangulate_batch, lds);
  if (e != hipSuccess) return e;
  TriK Kc;
  for (int i = 0; i < 9; i++) Kc.K[i] = K[i];
  hipLaunchKernelGGL(k_triangulate_batch, dim3(npairs), dim3(SCALE_THREADS), lds, s, cap, d_counts, d_kp, d_match,
                     d_pose, Kc, d_xyz, d_valid, d_mq, d_mt, d_npts);
  return hipGetLastError();
}

hipError_t orbx_launch_triangulate_host(hipStream_t s, int n, const float* d_p1, const float* d_p2, const double* K,
                                        const double* R, const double* t, float* d_xyz, uint8_t* d_valid) {
  if (n <= 0) return hipSuccess;
  TriP Pc;
  tri_projections(K, R, t, Pc.P, Pc.P + 12);
  hipLaunchKernelGGL(k_triangulate_host, dim3((n + SCALE_THREADS - 1) / SCALE_THREADS), dim3(SCALE_THREADS), 0, s, n,
                     d_p1, d_p2, Pc, d_xyz, d_valid);
  return hipGetLastError();
}

hipError_t orbx_launch_scale_join(hipStream_t s, int npairs, int chain, int cap, const int32_t* d_npts, const int32_t* d_mq,
                                  const int32_t* d_mt, const float* d_xyz, const uint8_t* d_valid,
                                  const OrbxPoseOut* d_pose, OrbxScaleOut* d_out) {
  if (npairs <= 0) return hipSuccess;
  if (chain < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)cap * 16;
  hipError_t e = allow_lds(k_scale_join, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scale_join, dim3(npairs), dim3(SCALE_THREADS), lds, s, cap, chain, d_npts, d_mq, d_mt, d_xyz,
                     d_valid, d_pose, d_out);
  return hipGetLastError();
}

hipError_t orbx_launch_scale_aligned(hipStream_t s, int n_prev, int n_cur, const float* d_prev,
                                     const uint8_t* d_prev_valid, const float* d_cur, const uint8_t* d_cur_valid,
                                     OrbxScaleOut* d_out) {
  const int m = n_prev < n_cur ? n_prev : n_cur;
  const size_t lds = (size_t)(m > 0 ? m : 1) * 8;
  hipError_t e = allow_lds(k_scale_aligned, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scale_aligned, dim3(1), dim3(SCALE_THREADS), lds, s, n_prev, n_cur, d_prev, d_prev_valid, d_cur,
                     d_cur_valid, d_out);
  return hipGetLastError();
}
